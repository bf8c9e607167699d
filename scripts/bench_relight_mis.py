"""The relighter's third strategy on one MI355X (HIP events, median over --reps after a warm-up, with minimum and maximum; comparisons
alternated in one process on the same inputs):
  * nero_env_cdf, the light table, at 512 x 1024 and at 2048 x 4096;
  * nero_bvh_relight_mis at (96, 96, 64) against nero_bvh_relight at (128, 128) on the same 4096 points -- 1 M (point, sample) lanes each --
    of a bumpy icosphere of 327 680 triangles, under both maps: ms and rays/s.  A light sample costs log2 gh + log2 gw dependent 8-byte
    loads of the table, every other sample two; the large table is 64 MB, beyond L2;
  * error at equal time: a 256 x 256 view under the 2048 x 4096 map with a sun-sized hot spot (a disk of 3 texels' radius at 50 000 x),
    linear RMSE over the hit pixels against a (4096, 4096) two-strategy render, for (128, 128) and for MIS sample counts scaled until its
    render takes the same time.
Prints one JSON line and writes it to profiles/bench_relight_mis.json.

    python scripts/bench_relight_mis.py [--reps 7] [--no-write]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(fns, reps, warmup=2):
    """the callables of `fns` in turn, reps + warmup rounds -> (median, min, max) ms of each (HIP events)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = [[] for _ in fns]
    for it in range(reps + warmup):
        for k, fn in enumerate(fns):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    return [(round(statistics.median(m), 4), round(min(m), 4), round(max(m), 4)) for m in ms]


def sun_map(h, w, g):
    env = torch.from_numpy(g.uniform(0.2, 1.2, (h, w, 3)).astype(np.float32))
    r0, c0, rad = int(h * 0.3), int(w * 0.6), 3.0 * h / 2048
    rr, cc = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    env[((rr - r0) ** 2 + (cc - c0) ** 2).float() <= max(rad, 0.5) ** 2] *= 50000.0
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-write', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight as RL
    from nero_amd.synthetic import icosphere
    dev = torch.device('cuda', 0)
    v, f = icosphere(7, 0.5, 0.15)
    g = np.random.default_rng(0)
    mats = {'metallic': g.uniform(0, 1, (len(v), 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (len(v), 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (len(v), 3)).astype(np.float32)}
    maps = {'512x1024': sun_map(512, 1024, g).to(dev), '2048x4096': sun_map(2048, 4096, g).to(dev)}
    rl = RL.Relighter(v, f, mats, maps['2048x4096'], convention='blender')
    tr = rl.tracer
    out = {'mesh_triangles': int(len(f)), 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}

    # ---- the table ---------------------------------------------------------------------------------------------------------------------
    out['table_build'] = {}
    for name, env in maps.items():
        (m, lo, hi), = alternate([lambda: RL.light_table(env, 2)], a.reps)
        info = RL.light_table(env, 2).info.cpu().tolist()
        out['table_build'][name] = {'ms': m, 'ms_min_max': [lo, hi], 'table_MB': round(env.shape[0] * env.shape[1] * 8 / 2 ** 20, 1),
                                    'zero_weight_cells': info[1], 'weight_bits': info[3]}

    # ---- the kernels, 1 M lanes each -----------------------------------------------------------------------------------------------------
    P = 4096
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(8, 0.0, 30.0, 3.0))[3]
    ro, rd = rl.camera_rays(pose, RL.default_K(800, 800), 800, 800)
    sf = rl.surface(ro, rd)
    sel = torch.linspace(0, sf['idx'].numel() - 1, P, device=dev).long()
    idx = sf['idx'][sel]
    rand_d, rand_s = RL.pixel_rotations(idx, 0)
    pt = RL.point_records(sf['pts'][sel], -rd[idx], sf['normal'][sel], RL.estimator_materials(sf['mat5'][sel]), rand_d, rand_s)
    rand_l = RL.pixel_shifts(idx, 0)
    tabs = {n: RL.sample_table(n, dev) for n in (64, 96, 128)}
    out['kernels_1M_lanes'] = {}
    for name, env in maps.items():
        table = RL.light_table(env, 2)
        two = lambda: RL.relight_points(tr, pt, tabs[128], tabs[128], env, 2)
        mis = lambda: RL.relight_points(tr, pt, tabs[96], tabs[96], env, 2, tab_l=tabs[64], rand_l=rand_l, table=table)
        (tm, t0, t1), (mm, m0, m1) = alternate([two, mis], a.reps)
        out['kernels_1M_lanes'][name] = {
            'points': P, 'two_strategy_samples': [128, 128], 'two_strategy_ms': tm, 'two_strategy_ms_min_max': [t0, t1],
            'two_strategy_Mrays_per_s': round(P * 256 / tm / 1e3, 1), 'mis_samples': [96, 96, 64], 'mis_ms': mm, 'mis_ms_min_max': [m0, m1],
            'mis_Mrays_per_s': round(P * 256 / mm / 1e3, 1), 'mis_over_two_strategy': round(mm / tm, 4)}

    # ---- error at equal time -------------------------------------------------------------------------------------------------------------
    K, hw = RL.default_K(256, 256), 256
    truth = rl.render(pose, K, hw, hw, samples=(4096, 4096))
    hit = truth['alpha'][..., 0] > 0
    rmse = lambda img: float(torch.sqrt(((img['rgb_lin'] - truth['rgb_lin'])[hit] ** 2).mean()))
    rl.light_table(None)                                                                # built once per map, outside the timed renders
    two = lambda: rl.render(pose, K, hw, hw, samples=(128, 128))
    counts = [96, 96, 64]
    for _ in range(3):                                                                  # scale the MIS counts to the two-strategy render's time
        mis = lambda: rl.render(pose, K, hw, hw, samples=tuple(counts))
        (tm, t0, t1), (mm, m0, m1) = alternate([two, mis], a.reps)
        if abs(mm / tm - 1.0) < 0.03:
            break
        counts = [max(1, int(round(n * tm / mm))) for n in counts]
    out['error_at_equal_time_256x256'] = {
        'hit_pixels': int(hit.sum()), 'mean_radiance': round(float(truth['rgb_lin'][hit].mean()), 4), 'truth_samples': [4096, 4096],
        'two_strategy_samples': [128, 128], 'two_strategy_ms': tm, 'two_strategy_ms_min_max': [t0, t1], 'two_strategy_rmse': round(rmse(two()), 5),
        'mis_samples': counts, 'mis_ms': mm, 'mis_ms_min_max': [m0, m1], 'mis_rmse': round(rmse(mis()), 5)}
    line = json.dumps(out)
    print(line)
    if not a.no_write:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'bench_relight_mis.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
