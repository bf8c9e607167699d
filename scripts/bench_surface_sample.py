"""Surface sampling on one MI355X (nero_amd/surface.py): the cdf (nero_surface_cdf), the samples (nero_surface_sample; both HIP events) and the
whole sample_surface call from a device-resident mesh (wall clock: it holds the read-back of the 32-byte record) at --n samples, on the
marching-cubes meshes of the model bench.py's inference_bench uses (scripts/bench_mesh.py) and on the white-noise mesh of
scripts/bench_mesh_clean.py.  Beside them the numpy route on the host in the same process: copy the mesh to the host, float64 areas, cumsum,
searchsorted, the barycentric mix, copy the points back.  The two sides ALTERNATE, --reps rounds after one warm-up round; every figure is
the median with [min, max].  Prints one JSON line and writes it to profiles/bench_surface_sample.json.  Nothing is asserted about the times.

    python scripts/bench_surface_sample.py [--res 256 512] [--noise 160] [--n 500000] [--reps 7] [--no-write]

Bytes of the kernels, from the shapes (T triangles, n samples): the cdf reads tris and three vertices per triangle (12 T + 36 T), writes and
rereads the doubled areas (8 T + 8 T), writes the weights (8 T) and scans them (8 T + 8 T); a sample walks bit_length(T) words of the cdf
(8 each), reads one triangle (12 + 36) and writes a point (12)."""
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
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def host_route(verts, tris, n, seed):
    """the mesh to the host; areas, cumsum, searchsorted and the barycentric mix in numpy; the points back"""
    v, f = verts.cpu().numpy().astype(np.float64), tris.cpu().numpy()
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cdf = np.cumsum(np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1))
    rg = np.random.default_rng(seed)
    face = np.minimum(np.searchsorted(cdf, rg.random(n) * cdf[-1], side='right'), len(f) - 1)
    su, r2 = np.sqrt(rg.random(n))[:, None], rg.random(n)[:, None]
    pts = (1 - su) * p0[face] + su * (1 - r2) * p1[face] + su * r2 * p2[face]
    return torch.from_numpy(pts.astype(np.float32)).to(verts.device)


def spread(xs):
    return {'median': round(statistics.median(xs), 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4)}


def measure(verts, tris, n, reps):
    from nero_amd import _lib as L
    from nero_amd import surface as S
    V, T, dev = verts.shape[0], tris.shape[0], verts.device
    ws = torch.empty(int(L.lib.nero_surface_cdf_workspace_bytes(T)), dtype=torch.uint8, device=dev)
    cdf = torch.empty(T, dtype=torch.int64, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    rows = {'cdf_ms': [], 'sample_ms': [], 'sample_surface_ms': [], 'host_route_ms': []}
    for it in range(reps + 1):                                         # (round 0: code objects, allocator, numpy's first touch)
        s = L.stream_ptr()
        ev[0].record()
        L.check(L.lib.nero_surface_cdf(L.ptr(verts), V, L.ptr(tris), T, L.ptr(ws), L.ptr(cdf), L.ptr(info), s))
        ev[1].record()
        L.check(L.lib.nero_surface_sample(L.ptr(verts), V, L.ptr(tris), T, L.ptr(cdf), L.ptr(info), 0, n, n, it, 1, L.ptr(pts), None, None, None, s))
        ev[2].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.sample_surface(verts, tris, n, seed=it)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host_route(verts, tris, n, it)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= 1:
            rows['cdf_ms'].append(ev[0].elapsed_time(ev[1]))
            rows['sample_ms'].append(ev[1].elapsed_time(ev[2]))
            rows['sample_surface_ms'].append((t1 - t0) * 1e3)
            rows['host_route_ms'].append((t2 - t1) * 1e3)
    out = {'V': V, 'T': T, 'n': n, 'reps': reps, 'workspace_bytes': ws.numel(),
           'bytes': {'cdf': 96 * T, 'sample': n * (8 * max(T - 1, 1).bit_length() + 60)}}
    out.update({k: spread(x) for k, x in rows.items()})
    out['host_over_device'] = round(out['host_route_ms']['median'] / out['sample_surface_ms']['median'], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--noise', type=int, default=160, help='edge of the white-noise grid of the last row (0: skip it)')
    ap.add_argument('--n', type=int, default=500000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    from bench_mesh import model
    from nero_amd import mesh as M
    dev = torch.device('cuda:0')
    net = model(dev)
    out = {'metric': 'surface_sample', 'device': torch.cuda.get_device_name(0)}
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        out[f'{res}^3'] = measure(verts, tris, args.n, args.reps)
        del verts, tris
        torch.cuda.empty_cache()
    if args.noise:
        g = torch.Generator(device=dev).manual_seed(6033)
        u = torch.rand((args.noise,) * 3, generator=g, device=dev) * 2 - 1
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        out[f'noise_{args.noise}^3'] = measure(verts, tris, args.n, args.reps)
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_surface_sample.json'), 'w') as fh_:
            fh_.write(line + '\n')


if __name__ == '__main__':
    main()
