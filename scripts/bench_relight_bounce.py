"""The relighter's one bounce on one MI355X (HIP events, median over --reps after a warm-up, with minimum and maximum; comparisons
alternated in one process on the same inputs).  The mesh is concave: the bumpy icosphere of bench_relight_mis.py (327 680 triangles, bumps
that shadow one another) standing in a bowl -- the lower half of a larger sphere, wound inwards -- so that a good part of the sample
directions meets the mesh.  One mesh, one map (512 x 1024, mild): the figures say nothing about other shapes.
  * nero_bvh_relight_bounce at (128, 128) against nero_bvh_relight at (128, 128), and nero_bvh_relight_mis_bounce at (96, 96, 64) against
    nero_bvh_relight_mis, on the same 4096 points -- 1 M (point, sample) lanes each: ms, the ratio, the share of lanes that bounce and the
    share of WAVEFRONTS in which at least one lane does (those walk twice: the divergence the kernel does not compact away);
  * one whole 256 x 256 view with and without the bounce;
  * linear RMSE over the hit pixels against a (4096, 4096) bounces=1 render, for bounces=1 at (128, 128) and at (68, 68, 46).
Nothing is asserted on times.  Prints one JSON line and writes it to profiles/bench_relight_bounce.json.

    python scripts/bench_relight_bounce.py [--reps 7] [--no-write]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_relight_mis import alternate  # noqa: E402


def concave_mesh():
    """the bumpy icosphere inside an inward-wound bowl (the lower half of an icosphere of radius 1.1, moved up so its rim is level with the
    inner sphere's centre) -> vertices float32, triangles int32"""
    from nero_amd.synthetic import icosphere
    v, f = icosphere(7, 0.5, 0.15)
    bv, bf = icosphere(4, 1.1)
    low = (bv[bf].mean(1)[:, 2] < 0.0)
    bf = bf[low][:, ::-1]                                                  # inward winding
    used, inv = np.unique(bf.reshape(-1), return_inverse=True)
    return (np.concatenate([v, bv[used]]).astype(np.float32), np.concatenate([f, inv.reshape(-1, 3) + len(v)]).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-write', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight as RL
    dev = torch.device('cuda', 0)
    v, f = concave_mesh()
    g = np.random.default_rng(0)
    mats = {'metallic': g.uniform(0, 1, (len(v), 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (len(v), 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (len(v), 3)).astype(np.float32)}
    env = torch.from_numpy(g.uniform(0.2, 1.2, (512, 1024, 3)).astype(np.float32)).to(dev)
    env[100:140, 300:380] *= 20.0                                          # a window, not a sun: the RMSE is not about fireflies here
    rl = RL.Relighter(v, f, mats, env, convention='blender')
    tr = rl.tracer
    out = {'mesh_triangles': int(len(f)), 'map': [512, 1024], 'reps': a.reps, 'device': torch.cuda.get_device_name(0)}

    # ---- the kernels, 1 M lanes each -----------------------------------------------------------------------------------------------------
    P = 4096
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(8, 0.0, 30.0, 3.0))[3]
    ro, rd = rl.camera_rays(pose, RL.default_K(800, 800), 800, 800)
    sf = rl.surface(ro, rd)
    sel = torch.linspace(0, sf['idx'].numel() - 1, P, device=dev).long()
    idx = sf['idx'][sel]
    rand_d, rand_s = RL.pixel_rotations(idx, 0)
    pt = RL.point_records(sf['pts'][sel], -rd[idx], sf['normal'][sel], RL.estimator_materials(sf['mat5'][sel]), rand_d, rand_s)
    rand_l, key = RL.pixel_shifts(idx, 0), RL.pixel_keys(idx, 0)
    tabs = {n: RL.sample_table(n, dev) for n in (64, 96, 128)}
    table = rl.light_table(None)
    mesh = (rl.verts, rl.tris.int(), rl.mat5, None)
    out['kernels_1M_lanes'] = {}
    for name, (td, ts, kw) in {'two_strategy_128_128': (tabs[128], tabs[128], {}),
                               'mis_96_96_64': (tabs[96], tabs[96], dict(tab_l=tabs[64], rand_l=rand_l, table=table))}.items():
        plain = lambda: RL.relight_points(tr, pt, td, ts, env, 2, **kw)
        bounce = lambda: RL.relight_points(tr, pt, td, ts, env, 2, bounces=1, mesh=mesh, key=key, **kw)
        (pm, p0, p1), (bm, b0, b1) = alternate([plain, bounce], a.reps)
        state = RL.relight_bounce_rays(tr, pt, td, ts, mesh, key, 0, **kw)['state'].reshape(P, -1)
        hit = state >= 2
        waves = hit.reshape(P, -1, 64).any(-1)                             # D = 256: four whole wavefronts per point
        direct, ind = plain(), bounce()
        out['kernels_1M_lanes'][name] = {
            'points': P, 'no_bounce_ms': pm, 'no_bounce_ms_min_max': [p0, p1], 'bounce_ms': bm, 'bounce_ms_min_max': [b0, b1],
            'bounce_over_no_bounce': round(bm / pm, 4), 'bounced_lane_share': round(float(hit.float().mean()), 4),
            'wavefronts_with_a_bounced_lane_share': round(float(waves.float().mean()), 4),
            'second_sample_dead_share_of_bounced': round(float((state == 3).float().sum() / hit.float().sum().clamp(min=1)), 4),
            'direct_terms_bit_equal': bool(torch.equal(direct[1], ind[1]) and torch.equal(direct[2], ind[2])),
            'mean_indirect_over_mean_rgb': round(float(ind[3].mean() / ind[0].mean()), 4)}

    # ---- one whole view, and the error against a long render ----------------------------------------------------------------------------------
    K, hw = RL.default_K(256, 256), 256
    view0 = lambda: rl.render(pose, K, hw, hw, samples=(128, 128))
    view1 = lambda: rl.render(pose, K, hw, hw, samples=(128, 128), bounces=1)
    (vm0, v00, v01), (vm1, v10, v11) = alternate([view0, view1], a.reps)
    truth = rl.render(pose, K, hw, hw, samples=(4096, 4096), bounces=1)
    hit = truth['alpha'][..., 0] > 0
    rmse = lambda img: round(float(torch.sqrt(((img['rgb_lin'] - truth['rgb_lin'])[hit] ** 2).mean())), 5)
    out['view_256x256'] = {
        'hit_pixels': int(hit.sum()), 'no_bounce_128_128_ms': vm0, 'no_bounce_ms_min_max': [v00, v01], 'bounce_128_128_ms': vm1,
        'bounce_ms_min_max': [v10, v11], 'truth_samples': [4096, 4096], 'mean_radiance': round(float(truth['rgb_lin'][hit].mean()), 4),
        'mean_indirect': round(float(truth['indirect_lin'][hit].mean()), 4), 'rmse_bounces1_128_128': rmse(view1()),
        'rmse_bounces1_68_68_46': rmse(rl.render(pose, K, hw, hw, samples=(68, 68, 46), bounces=1)), 'rmse_bounces0_128_128': rmse(view0())}
    line = json.dumps(out)
    print(line)
    if not a.no_write:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'bench_relight_bounce.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
