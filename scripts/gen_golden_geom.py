"""Writes tests/golden/geom_eval.npz: what the UNMODIFIED reference computes for the pieces of its Chamfer procedure that run without
nvdiffrast / open3d (through oracle/ref_shim, on the CPU).  Data only; runs where a reference checkout exists (NERO_REFERENCE_ROOT).

  views      3 seeded look_at_pose views of 64 x 48 pixels: analytic sphere depth maps (radius 0.5, float32) + masks, K, poses (float64)
  ref_pts_i  utils.base_utils: pose_apply(pose_inverse(pose), mask_depth_to_pts(mask, depth, K)).astype(float32)
  nn_*       two seeded clouds of 20 000 / 30 000 points near a sphere of radius 0.5 (64 exact duplicates of cloud b inside cloud a) and
             eval_synthetic_shape.nearest_dist(a, b), nearest_dist(b, a)

    python scripts/gen_golden_geom.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_VIEWS, H, W, FOCAL = 3, 48, 64, 60.0
N_A, N_B, N_DUP = 20000, 30000, 64


def views():
    from nero_amd.synthetic import look_at_pose
    rg = np.random.default_rng(11)
    az = rg.uniform(0, 2 * np.pi, N_VIEWS)
    el = rg.uniform(0.15, 1.2, N_VIEWS)
    cams = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1) * 3.0
    poses = np.stack([look_at_pose(c) for c in cams], 0).astype(np.float64)
    Ks = np.stack([np.array([[FOCAL * (1 + 0.05 * i), 0, W / 2 - 0.7 * i], [0, FOCAL * (1 + 0.03 * i), H / 2 + 0.4 * i], [0, 0, 1]], np.float64)
                   for i in range(N_VIEWS)], 0)
    return poses, Ks


def clouds():
    rg = np.random.default_rng(12)

    def near_sphere(n):
        p = rg.normal(size=(n, 3))
        p = p / np.linalg.norm(p, axis=1, keepdims=True) * (0.5 + 0.004 * rg.normal(size=(n, 1)))
        return p.astype(np.float32)
    a, b = near_sphere(N_A), near_sphere(N_B)
    dup = rg.choice(N_A, N_DUP, replace=False)
    a[dup] = b[rg.choice(N_B, N_DUP, replace=False)]
    return a, b, np.sort(dup)


def main():
    from tests import geom_ref
    poses, Ks = views()
    a, b, dup = clouds()
    from oracle import ref_shim
    cwd = os.getcwd()
    ref_shim.install(force_cpu=True)
    import tqdm
    tqdm.tqdm = lambda it=None, *x, **k: it
    from utils.base_utils import mask_depth_to_pts, pose_apply, pose_inverse
    import eval_synthetic_shape as ess
    ess.tqdm = lambda it=None, *x, **k: it
    out = {'poses': poses, 'Ks': Ks, 'hw': np.array([H, W]), 'nn_a': a, 'nn_b': b, 'nn_dup': dup}
    for i in range(N_VIEWS):
        depth, mask = geom_ref.sphere_depth(Ks[i], poses[i], H, W, 0.5)
        pts = pose_apply(pose_inverse(poses[i]), mask_depth_to_pts(mask, depth, Ks[i]))
        assert pts.dtype == np.float64
        out[f'depth_{i}'], out[f'mask_{i}'], out[f'ref_pts_{i}'] = depth, mask, pts.astype(np.float32)
    out['nn_ab'] = ess.nearest_dist(a, b, 1024)
    out['nn_ba'] = ess.nearest_dist(b, a, 1024)
    assert out['nn_ab'].dtype == np.float32
    os.chdir(cwd)
    path = os.path.join(ROOT, 'tests', 'golden', 'geom_eval.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
