"""The relighter on one MI355X, each comparison alternated in one process on the same inputs (HIP events, median over --reps after a
warm-up, with minimum and maximum):
  * nero_bvh_relight (rays made, cast, lit and weighed in one kernel + the finishing pass) against the composed route on the same 1 M rays
    (4096 points x 128 + 128 samples): nero_relight_rays, nero_bvh_occluded, nero_env_lookup and a torch masked sum per point.  The composed
    route stores and re-reads about 60 bytes per ray that the fused kernel never moves, and it does NOT evaluate the BRDF weights: it is a
    lower bound of a composed relighter;
  * nero_bvh_trace_faces against nero_bvh_trace on 1 M camera rays;
  * one whole 800 x 800 view (Relighter.render) at 128 + 128 and 512 + 512 samples: wall time, the minimum of two runs after one warm-up run,
    all samples listed.
The mesh is a bumpy icosphere of 81 920 triangles (nero_amd.synthetic.icosphere(6, 0.5, 0.15)), the map a 256 x 512 random one with a hot
texel.  Prints one JSON line and writes it to profiles/bench_relight.json.

    python scripts/bench_relight.py [--reps 7] [--views 128 512] [--no-write]"""
import argparse
import json
import os
import statistics
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--views', type=int, nargs='*', default=[128, 512])
    ap.add_argument('--no-write', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight as RL
    from nero_amd.synthetic import icosphere
    dev = torch.device('cuda', 0)
    v, f = icosphere(6, 0.5, 0.15)
    g = np.random.default_rng(0)
    mats = {'metallic': g.uniform(0, 1, (len(v), 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (len(v), 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (len(v), 3)).astype(np.float32)}
    env = torch.from_numpy(g.uniform(0.2, 1.2, (256, 512, 3)).astype(np.float32))
    env[60, 300] *= 1000.0
    rl = RL.Relighter(v, f, mats, env, convention='blender')
    tr = rl.tracer
    out = {'mesh_triangles': int(len(f)), 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}

    # ---- fused against composed, 1 M rays --------------------------------------------------------------------------------------------
    P, Dd, Ds = 4096, 128, 128
    D = Dd + Ds
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(8, 0.0, 30.0, 3.0))[3]
    ro, rd = rl.camera_rays(pose, RL.default_K(800, 800), 800, 800)
    sf = rl.surface(ro, rd)
    sel = torch.linspace(0, sf['idx'].numel() - 1, P, device=dev).long()
    idx = sf['idx'][sel]
    rand_d, rand_s = RL.pixel_rotations(idx, 0)
    pt = RL.point_records(sf['pts'][sel], -rd[idx], sf['normal'][sel], RL.estimator_materials(sf['mat5'][sel]), rand_d, rand_s)
    tab_d, tab_s = RL.sample_table(Dd, dev), RL.sample_table(Ds, dev)
    fused_out = []

    def fused():
        fused_out[:] = RL.relight_points(tr, pt, tab_d, tab_s, rl.env, 2)

    composed_out = []

    def composed():
        o, d, dead = RL.relight_rays(pt, tab_d, tab_s, 0)
        blocked = tr.occluded(o, d, skip=dead)
        L = RL.env_lookup(rl.env, d, 2)
        lit = ((blocked | dead) == 0).float()[:, None]
        composed_out[:] = [(L * lit).reshape(P, D, 3)[:, :Dd].mean(1)]
    (fm, f0, f1), (cm, c0, c1) = alternate([fused, composed], a.reps)
    # with metallic 0 the two diffuse means would agree; here only the lit fraction is compared
    out['fused_vs_composed_1M_rays'] = {
        'points': P, 'samples': [Dd, Ds], 'fused_ms': fm, 'fused_ms_min_max': [f0, f1], 'composed_ms': cm, 'composed_ms_min_max': [c0, c1],
        'fused_over_composed': round(fm / cm, 4),
        'note': 'composed = nero_relight_rays + nero_bvh_occluded + nero_env_lookup + torch masked mean; it evaluates no BRDF weight'}

    # ---- trace_faces against trace, 1 M camera rays ----------------------------------------------------------------------------------
    ro1, rd1 = rl.camera_rays(pose, RL.default_K(1024, 1024), 1024, 1024)
    (tm, t0, t1), (gm, g0, g1) = alternate([lambda: tr.trace(ro1, rd1), lambda: RL.trace_faces(tr, ro1, rd1)], a.reps)
    depth = tr.trace(ro1, rd1)[2]
    out['trace_faces_vs_trace_1M_camera_rays'] = {
        'trace_ms': tm, 'trace_ms_min_max': [t0, t1], 'trace_faces_ms': gm, 'trace_faces_ms_min_max': [g0, g1],
        'trace_faces_over_trace': round(gm / tm, 4), 'hit_share': round(float((depth < 10).float().mean()), 4)}

    # ---- whole views -----------------------------------------------------------------------------------------------------------------
    views = {}
    for s in a.views:
        runs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            img = rl.render(pose, RL.default_K(800, 800), 800, 800, samples=(s, s))
            torch.cuda.synchronize()
            runs.append(round((time.perf_counter() - t) * 1e3, 2))
        hit = int((img['alpha'] > 0).sum())
        views[f'{s}+{s}'] = {'ms_min_of_2_after_warmup': min(runs[1:]), 'ms_all_runs': runs, 'hit_pixels': hit,
                             'shadow_rays': hit * 2 * s, 'Mrays_per_s': round(hit * 2 * s / min(runs[1:]) / 1e3, 1)}
    out['view_800x800'] = views
    line = json.dumps(out)
    print(line)
    if not a.no_write:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'bench_relight.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
