"""Vertex normals on one MI355X (nero_amd.mesh.vertex_normals, nero_amd/csrc/mesh_normals.hip): the nero_vertex_normals call from a
device-resident mesh (HIP events) for both weights, on the marching-cubes meshes of the model bench.py's inference_bench uses
(scripts/bench_mesh.py) and on the white-noise mesh of scripts/bench_mesh_clean.py.  Beside it two routes that sum in floating point, so
neither gives the same bits from run to run or for another order of the triangles: torch's index_add_ on the same GPU (float64, wall clock
around a synchronise) and numpy's np.add.at on the host (mesh to the host, normals back).  The three ALTERNATE, --reps rounds after one
warm-up round; every figure is the median with [min, max].  The launches of one call (clear, max, add, finish) are timed apart by
torch.profiler in one further call per weight.  Prints one JSON line and writes it to profiles/bench_vertex_normals.json.  Nothing is
asserted about the times.

    python scripts/bench_vertex_normals.py [--res 256 512] [--noise 160] [--reps 5] [--no-write]

Bytes of the kernels, from the shapes (V vertices, T triangles): a pass over the faces reads tris and three vertices per triangle (12 T + 36
T); the add pass also sends nine 8-byte atomic adds per face (72 T); the workspace is cleared (24 V) and the finish pass reads it and writes
the normals (24 V + 12 V).  The max pass runs in area mode only."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def _terms(xp, p, weight):
    """per face and corner, the float64 contribution [T,3,3] in the array library xp (numpy or torch)"""
    cross = np.cross if xp is np else torch.linalg.cross
    c = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    if weight == 'area':
        return xp.stack([c, c, c], 1)
    if xp is np:
        with np.errstate(all='ignore'):
            n = np.nan_to_num(c / ((c * c).sum(1) ** 0.5)[:, None])    # (a face without area: no direction, no contribution)
    else:
        n = torch.nan_to_num(c / ((c * c).sum(1) ** 0.5)[:, None])
    out = []
    for i in range(3):
        a, b = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        x = cross(a, b)
        theta = (xp.arctan2 if xp is np else torch.atan2)((x * x).sum(1) ** 0.5, (a * b).sum(1))
        out.append(theta[:, None] * n)
    return xp.stack(out, 1)


def torch_route(verts, tris, weight):
    """float64 on the device: index_add_ per corner"""
    t = tris.long()
    terms = _terms(torch, verts.double()[t], weight)
    s = torch.zeros(verts.shape[0], 3, dtype=torch.float64, device=verts.device)
    for i in range(3):
        s.index_add_(0, t[:, i], terms[:, i])
    return torch.nn.functional.normalize(s, dim=1).float()


def host_route(verts, tris, weight):
    """the mesh to the host, np.add.at per corner, the normals back"""
    v, f = verts.cpu().numpy().astype(np.float64), tris.cpu().numpy()
    terms = _terms(np, v[f], weight)
    s = np.zeros((len(v), 3))
    for i in range(3):
        np.add.at(s, f[:, i], terms[:, i])
    with np.errstate(all='ignore'):
        n = np.nan_to_num(s / np.linalg.norm(s, axis=1, keepdims=True))
    return torch.from_numpy(n.astype(np.float32)).to(verts.device)


def spread(xs):
    return {'median': round(statistics.median(xs), 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4)}


def phases(call):
    """device time of every launch of one call, by kernel name, in microseconds (torch.profiler)"""
    from torch.profiler import ProfilerActivity, profile
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    rows = {}
    for k in prof.key_averages():
        t = getattr(k, 'self_device_time_total', None)
        t = float(getattr(k, 'self_cuda_time_total', 0.0) if t is None else t)
        name = re.search(r'normals_\w+|[Mm]emset', k.key)
        if t > 0 and name:
            rows[name.group(0)] = round(rows.get(name.group(0), 0.0) + t, 2)
    return rows


def measure(verts, tris, reps):
    from nero_amd import _lib as L
    from nero_amd import mesh as M
    V, T, dev = verts.shape[0], tris.shape[0], verts.device
    ws = torch.empty(int(L.lib.nero_vertex_normals_workspace_bytes(V, T)), dtype=torch.uint8, device=dev)
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {'V': V, 'T': T, 'reps': reps, 'workspace_bytes': ws.numel(),
           'bytes': {'area': 2 * 48 * T + 72 * T + 60 * V, 'angle': 48 * T + 72 * T + 60 * V}}
    for weight in ('area', 'angle'):
        call = lambda: L.check(L.lib.nero_vertex_normals(L.ptr(verts), V, L.ptr(tris), T, M.NORMAL_WEIGHTS[weight], L.ptr(ws), L.ptr(normals),
                                                         L.ptr(info), L.stream_ptr()))
        rows = {'call_ms': [], 'vertex_normals_ms': [], 'torch_index_add_ms': [], 'host_add_at_ms': []}
        for it in range(reps + 1):                                     # (round 0: code objects, allocator, numpy's first touch)
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mine = M.vertex_normals(verts, tris, weight=weight)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            theirs = torch_route(verts, tris, weight)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host_route(verts, tris, weight)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if it >= 1:
                rows['call_ms'].append(ev[0].elapsed_time(ev[1]))
                rows['vertex_normals_ms'].append((t1 - t0) * 1e3)
                rows['torch_index_add_ms'].append((t2 - t1) * 1e3)
                rows['host_add_at_ms'].append((t3 - t2) * 1e3)
        res = {k: spread(x) for k, x in rows.items()}
        res['gb_per_s'] = round(out['bytes'][weight] / (res['call_ms']['median'] * 1e-3) / 1e9, 1)
        res['largest_difference_from_torch'] = float((mine - theirs).abs().max())
        res['info'] = info.tolist()
        try:
            res['phases_us'] = phases(call)
        except Exception as e:                                         # noqa: BLE001 (a profiler that cannot trace here: said, not hidden)
            res['phases_us'] = f'unavailable: {type(e).__name__}: {e}'
        out[weight] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--noise', type=int, default=160, help='edge of the white-noise grid of the last row (0: skip it)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    from bench_mesh import model
    from nero_amd import mesh as M
    dev = torch.device('cuda:0')
    net = model(dev)
    out = {'metric': 'vertex_normals', 'device': torch.cuda.get_device_name(0)}
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        out[f'{res}^3'] = measure(verts, tris, args.reps)
        del verts, tris
        torch.cuda.empty_cache()
    if args.noise:
        g = torch.Generator(device=dev).manual_seed(6033)
        u = torch.rand((args.noise,) * 3, generator=g, device=dev) * 2 - 1
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        out[f'noise_{args.noise}^3'] = measure(verts, tris, args.reps)
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_vertex_normals.json'), 'w') as fh_:
            fh_.write(line + '\n')


if __name__ == '__main__':
    main()
