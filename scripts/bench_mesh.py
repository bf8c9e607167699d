"""Stage-I mesh extraction on one MI355X: the SDF grid (extract_fields), grid + HIP marching cubes (extract_geometry), and the marching-cubes
kernels alone (nero_mcubes_count + the 16-byte readback + nero_mcubes_emit, HIP events, median over --reps after a warm-up) on the model
bench.py's inference_bench uses (seed 6033, perturb_state at variance 0.5).  Prints one JSON line.

    python scripts/bench_mesh.py [--res 256 512] [--reps 20] [--kernels-only]

Bytes of the kernels, from the shapes (N grid points, V vertices, T triangles): the grid read once (4 N; the neighbour reads of the count
pass hit the caches), the one-byte point code written once and read by both emit passes (3 N), per vertex its 12-byte output and at most
one 4-byte vertex base written (16 V), per triangle its 12-byte output and three vertex-base reads (24 T)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.3          # achievable HBM rate of one MI355X (measuring guide), TB/s


def model(dev):
    from bench import BELL, VARIANCE
    from nero_amd.renderer import NeROShapeRenderer
    from nero_amd.synthetic import perturb_state
    torch.manual_seed(6033)
    net = NeROShapeRenderer(dict(BELL), training=False)
    perturb_state(net, VARIANCE)
    return net.to(dev)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernels(u, reps):
    """count + readback + emit on the device grid u, HIP events; -> dict"""
    import ctypes as C
    from nero_amd import _lib as L
    from nero_amd import mesh as M
    nx, ny, nz = u.shape
    ws = torch.empty(M.workspace_bytes(u.shape), dtype=torch.uint8, device=u.device)
    tot = torch.empty(2, dtype=torch.int64, device=u.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    rows = []
    for it in range(reps + 3):
        s = L.stream_ptr()
        ev[0].record()
        L.check(L.lib.nero_mcubes_count(L.ptr(u), nx, ny, nz, C.c_float(0.0), L.ptr(ws), L.ptr(tot), s))
        ev[1].record()
        V, T = tot.tolist()
        verts = torch.empty((V, 3), dtype=torch.float32, device=u.device)
        tris = torch.empty((T, 3), dtype=torch.int32, device=u.device)
        ev[2].record()
        L.check(L.lib.nero_mcubes_emit(L.ptr(u), nx, ny, nz, C.c_float(0.0), L.ptr(ws), L.ptr(verts), V, L.ptr(tris), T, s))
        ev[3].record()
        torch.cuda.synchronize()
        if it >= 3:                                                    # (warm-up: code objects, allocator)
            rows.append((ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), ev[0].elapsed_time(ev[3])))
        del verts, tris
    n = nx * ny * nz
    nbytes = 7 * n + 16 * V + 24 * T
    med = [statistics.median(r[i] for r in rows) for i in range(3)]
    return {'grid': f'{nx}x{ny}x{nz}', 'V': V, 'T': T, 'reps': reps, 'count_ms': round(med[0], 4), 'emit_ms': round(med[1], 4),
            'total_ms': round(med[2], 4), 'total_ms_min': round(min(r[2] for r in rows), 4), 'bytes': nbytes,
            'GBps': round(nbytes / (med[2] * 1e-3) / 1e9, 1), 'frac_of_hbm': round(nbytes / (med[2] * 1e-3) / (HBM_TBS * 1e12), 3),
            'workspace_bytes': M.workspace_bytes(u.shape)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernels-only', action='store_true', help='skip the end-to-end extract_fields / extract_geometry timings')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    net = model(dev)
    net.extract_geometry(resolution=64)                                # warm-up (packing, allocator, code objects)
    out = {'metric': 'stage1_mesh_extraction', 'device': torch.cuda.get_device_name(0), 'hbm_TBps_achievable': HBM_TBS}
    for res in args.res:
        r = {}
        if not args.kernels_only:
            d_f, _ = wall(lambda: net.extract_fields(resolution=res))
            d_g, (v, f) = wall(lambda: net.extract_geometry(resolution=res))
            r['extract_fields_s'] = round(d_f, 4)
            r['extract_geometry_s'] = round(d_g, 4)
            r['geometry_V'], r['geometry_T'] = len(v), len(f)
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        r['marching_cubes'] = kernels(u, args.reps)
        del u
        torch.cuda.empty_cache()
        out[f'{res}^3'] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
