"""The geometry evaluation (nero_amd/eval_shape.py, nero_amd/csrc/geom_eval.hip) on one MI355X: HIP events around the C-ABI calls on seeded
inputs, a warm-up, the median over --reps, a device synchronise before any clock is read.  Writes one JSON document (--out) and prints it.

    python scripts/bench_eval.py [--reps 20] [--out profiles/bench_eval.json] [--kernels-only]

  nearest_dist    50 000 x 50 000 (the synthetic procedure after down-sampling) and 500 000 x 500 000 (the real procedure's sample count):
                  time and pairs/s, against
                  * the ceiling 256 CUs x 4 SIMDs x 32 lanes per clock (a wave-64 VALU instruction issues over 2 cycles; x 2 flops this is
                    the chip's 157 TFLOP/s fp32 vector peak) x clock / VALU instructions per pair.  The kernel's inner loop holds 208 VALU
                    instructions per 32 pairs (96 v_sub, 32 v_mul, 64 v_fmac, 16 v_min3, counted in the compiled ISA), 6.5 per pair, fp32
                    unpacked by project rule; the clock is the chip's maximum, 2.4 GHz -- the clock held under this load is not measured here;
                  * the reference's formulation (eval_synthetic_shape.py:16-25: broadcast difference of a batch of 1024 against all of pts1,
                    norm, min) written in plain torch and run on the same GPU in the same process.
  voxel_down_sample   20 M points (about 128 views of 800 x 800 at a quarter coverage), voxel 0.01.
  depth view      one 800 x 800 view of a 327 680-triangle icosphere: rays + trace + depth, mask and points.
--kernels-only skips the torch baseline (for a rocprofv3 --kernel-trace --stats run of the kernels alone)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_PAIR = 208 / 32
MAX_CLOCK_HZ = 2.4e9
LANES = 256 * 4 * 32


def cloud(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, 3, generator=g)
    p = p / p.norm(dim=1, keepdim=True) * (0.5 + 0.004 * torch.randn(n, 1, generator=g))
    return p.to(dev).contiguous()


def timed(fn, reps, warmup=3):
    """-> list of milliseconds (HIP events, one synchronise per repetition)"""
    out = []
    for it in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(a.elapsed_time(b))
    return out


def torch_nearest_dist(p0, p1, batch=1024):
    """the reference's formulation, on device tensors"""
    dists = []
    for i in range(0, p0.shape[0], batch):
        dist = torch.norm(p0[i:i + batch, None, :] - p1[None, :, :], dim=-1)
        dists.append(torch.min(dist, 1)[0])
    return torch.cat(dists, 0)


def bench_nn(n, reps, dev, baseline):
    from nero_amd import _lib as L
    from nero_amd import eval_shape as E
    q, r = cloud(n, 1, dev), cloud(n, 2, dev)
    ws = torch.empty(int(L.lib.nero_nn_dist_workspace_bytes(n, n, 0)), dtype=torch.uint8, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    run = lambda: L.check(L.lib.nero_nn_dist(L.ptr(q), n, L.ptr(r), n, L.ptr(ws), 0, L.ptr(dist), None, L.stream_ptr()))
    ms = timed(run, reps)
    med = statistics.median(ms)
    pairs = float(n) * n
    ceiling = LANES * MAX_CLOCK_HZ / VALU_PER_PAIR
    out = {'nq': n, 'nr': n, 'splits': E.nn_splits(n, n), 'reps': reps, 'ms': round(med, 4), 'ms_min': round(min(ms), 4),
           'ms_max': round(max(ms), 4), 'pairs_per_s': round(pairs / (med * 1e-3), 0), 'valu_per_pair': VALU_PER_PAIR,
           'ceiling_pairs_per_s_at_2.4GHz': round(ceiling, 0), 'share_of_ceiling': round(pairs / (med * 1e-3) / ceiling, 3)}
    if baseline:
        b_reps = max(3, reps // 4) if n > 100000 else reps
        bms = timed(lambda: torch_nearest_dist(q, r), b_reps, warmup=1)
        bmed = statistics.median(bms)
        ref = torch_nearest_dist(q, r)
        out.update({'torch_baseline_ms': round(bmed, 3), 'torch_baseline_reps': b_reps, 'speedup_over_torch_baseline': round(bmed / med, 2),
                    'max_abs_diff_vs_baseline': float((ref - dist).abs().max())})
    return out


def bench_voxel(n, reps, dev):
    from nero_amd import _lib as L
    p = cloud(n, 3, dev)
    ws = torch.empty(int(L.lib.nero_voxel_downsample_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    out = torch.empty((1 << 20, 3), dtype=torch.float32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int64, device=dev)
    run = lambda: L.check(L.lib.nero_voxel_downsample(L.ptr(p), n, 0.01, L.ptr(ws), L.ptr(out), out.shape[0], L.ptr(n_out), L.stream_ptr()))
    ms = timed(run, reps, warmup=2)
    return {'points': n, 'voxel': 0.01, 'voxels': int(n_out), 'reps': reps, 'ms': round(statistics.median(ms), 3), 'ms_min': round(min(ms), 3),
            'workspace_bytes': ws.numel()}


def bench_view(reps, dev, res=800):
    from nero_amd import eval_shape as E
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import icosphere, look_at_pose
    v, f = icosphere(7, 0.5)
    rt = RayTracer(v, f)
    pose = look_at_pose(np.array([2.0, 1.5, 1.2])).astype(np.float64)
    K = np.array([[1100.0, 0, res / 2], [0, 1100.0, res / 2], [0, 0, 1]])
    ms = timed(lambda: E._view(rt, rt._v, pose, K, (res, res), 0.0, True), reps)
    pts = E._view(rt, rt._v, pose, K, (res, res), 0.0, True)[2]
    return {'view': f'{res}x{res}', 'triangles': int(len(f)), 'points': int(len(pts)), 'reps': reps, 'ms': round(statistics.median(ms), 3),
            'ms_min': round(min(ms), 3), 'note': 'rays + BVH trace + depth / mask / points, with the host read-back of the point count'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'bench_eval.json'))
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--voxel-points', type=int, default=20_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_eval.py measures on a GPU; none is visible')
    dev = torch.device('cuda:0')
    out = {'metric': 'geometry_evaluation', 'device': torch.cuda.get_device_name(0)}
    out['nearest_dist'] = [bench_nn(n, args.reps, dev, not args.kernels_only) for n in (50_000, 500_000)]
    out['voxel_down_sample'] = bench_voxel(args.voxel_points, max(3, args.reps // 4), dev)
    out['depth_view'] = bench_view(args.reps, dev)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
