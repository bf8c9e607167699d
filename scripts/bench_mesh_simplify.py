"""Simplification of the Stage-I mesh by vertex clustering on one MI355X: the count pass and the emit pass (HIP events, median over --reps
after a warm-up) and the whole simplify_mesh_device call (wall clock: it holds the read-backs, and for a face budget the counting passes of
the search), on the marching-cubes mesh of the model bench.py's inference_bench and scripts/bench_mesh.py use (seed 6033, perturb_state at
variance 0.5), at cell = 2 grid steps and at a budget of 100 000 faces.  Beside them the numpy restatement tests/mesh_simplify_ref.py on
the host of the same box in the same run, mesh copies included.  Prints one JSON line and writes it to profiles/bench_mesh_simplify.json.

    python scripts/bench_mesh_simplify.py [--res 256 512] [--reps 20] [--rays 1048576] [--bvh-build {host,device}] [--no-write]

Bytes of the kernels, from the shapes (V vertices, T triangles, C occupied cells, V' / S / T' output vertices, survivors, output faces):
count reads the vertices and writes keys and ids (24 V), reads tris and the keys of their corners and writes the flags (40 T), scans them
(8 T), sorts the 64-bit keys with their ids (8 radix passes of 24 V), flags and scans the heads and scatters the cell ids (32 V), flags the
used cells (28 T) and scans them (8 V).  emit writes and sorts the contribution keys (12 T read, 24 T written, 48 T per radix pass, one
pass per 8 bits of V), finds the runs (24 T), reads per contribution its triangle and three vertices (12 T of ids + 3 x 48 T), the sorted
vertices of the cells (16 V), writes the outputs (44 V'), the maps (12 V + 4 T), the triples and their two sorts (32 S + 24 S per pass of
the 64-bit key, 16 S per pass of the 32-bit key), the first-of-run flags and their scan (56 S) and the triangles (40 T + 12 T').

Only here: the BVH build and the trace of one fixed, seeded ray set (--rays rays from a sphere of radius 1.5 towards points in the unit
ball) against the original and against the simplified mesh -- what Stage II pays per step for the triangles it cannot resolve."""
import argparse
import ctypes as C
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
HBM_TBS = 6.3          # achievable HBM rate of one MI355X (measuring guide), TB/s


def bit_length(x):
    return int(x).bit_length()


def byte_model(V, T, V2, S, T2):
    count = 24 * V + 40 * T + 8 * T + 8 * 24 * V + 32 * V + 28 * T + 8 * V
    passes_v = (bit_length(V) + 7) // 8
    passes_o = (bit_length(V2) + 7) // 8
    emit = 36 * T + 48 * T * passes_v + 24 * T + 12 * T + 144 * T + 16 * V + 44 * V2 + 12 * V + 4 * T
    emit += 32 * S + 24 * S * (4 + passes_o) + 16 * S * passes_o + 56 * S + 40 * T + 12 * T2
    return {'count': count, 'emit': emit, 'total': count + emit}


def kernels(verts, tris, cell, reps):
    """count / emit on the device mesh, HIP events; -> dict"""
    from nero_amd import _lib as L
    V, T = verts.shape[0], tris.shape[0]
    dev = verts.device
    origin = (C.c_double * 3)(*verts.amin(dim=0).double().tolist())
    ws = torch.empty(int(L.lib.nero_mesh_simplify_workspace_bytes(V, T)), dtype=torch.uint8, device=dev)
    totals = torch.empty(4, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    fmap = torch.empty(T, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    rows = []
    for it in range(reps + 3):
        s = L.stream_ptr()
        ev[0].record()
        L.check(L.lib.nero_mesh_simplify_count(L.ptr(verts), L.ptr(tris), T, V, cell, origin, 1, L.ptr(ws), L.ptr(totals), s))
        ev[1].record()
        ev[2].record()
        L.check(L.lib.nero_mesh_simplify_count(L.ptr(verts), L.ptr(tris), T, V, cell, origin, 0, L.ptr(ws), L.ptr(totals), s))
        ev[3].record()
        V2, S, bad_v, bad_t = totals.tolist()
        assert bad_v == 0 and bad_t == 0
        pos = torch.empty((V2, 3), dtype=torch.float64, device=dev)
        v2 = torch.empty((V2, 3), dtype=torch.float32, device=dev)
        key = torch.empty(V2, dtype=torch.int64, device=dev)
        f2 = torch.empty((S, 3), dtype=torch.int32, device=dev)
        ev[4].record()
        L.check(L.lib.nero_mesh_simplify_emit(L.ptr(verts), L.ptr(tris), T, V, cell, origin, 1, 1, L.ptr(ws), L.ptr(pos), L.ptr(v2), L.ptr(key),
                                              V2, L.ptr(f2), S, L.ptr(vmap), L.ptr(fmap), L.ptr(n_out), s))
        ev[5].record()
        torch.cuda.synchronize()
        if it >= 3:                                                    # (warm-up: code objects, allocator)
            rows.append((ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), ev[4].elapsed_time(ev[5])))
        T2 = int(n_out.item())
        del pos, v2, key, f2
    med = [statistics.median(r[i] for r in rows) for i in range(3)]
    nb = byte_model(V, T, V2, S, T2)
    tot = med[1] + med[2]
    return {'cell': cell, 'V_out': V2, 'survivors': S, 'T_out': T2, 'reps': reps, 'count_faces_only_ms': round(med[0], 4),
            'count_ms': round(med[1], 4), 'emit_ms': round(med[2], 4), 'kernels_ms': round(tot, 4), 'bytes': nb,
            'GBps': round(nb['total'] / (tot * 1e-3) / 1e9, 1), 'frac_of_hbm': round(nb['total'] / (tot * 1e-3) / (HBM_TBS * 1e12), 4),
            'workspace_bytes': ws.numel()}


def wall_median(fn, reps):
    out = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if it >= 1:
            out.append(time.perf_counter() - t0)
    return statistics.median(out), r


def host_route(verts, tris, cell):
    """the mesh to the host, the numpy restatement, the result back"""
    from tests import mesh_simplify_ref as S
    o = S.simplify(verts.cpu().numpy(), tris.cpu().numpy(), cell)
    return torch.from_numpy(o['verts32']).to(verts.device), torch.from_numpy(o['tris']).to(verts.device)


def trace_cost(verts, tris, res, rays_o, rays_d, reps, bvh_build='host'):
    """BVH build (first use; bvh_build: by the host builder or on the device) and the trace of the fixed ray set, on the mesh mapped to the
    box [-1, 1]^3 -> dict"""
    from nero_amd.raytracing import RayTracer
    world = (verts / (res - 1.0) * 2.0 - 1.0).contiguous()
    t0 = time.perf_counter()
    tracer = RayTracer(world, tris, build=bvh_build)
    _, _, t = tracer.trace(rays_o[:64], rays_d[:64])                  # (the device BVH is built on first use)
    torch.cuda.synchronize()
    build = time.perf_counter() - t0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for it in range(reps + 2):
        ev[0].record()
        _, _, t = tracer.trace(rays_o, rays_d)
        ev[1].record()
        torch.cuda.synchronize()
        if it >= 2:
            ms.append(ev[0].elapsed_time(ev[1]))
    t = t.reshape(-1)
    return {'faces': int(tris.shape[0]), 'bvh_build': bvh_build, 'bvh_build_ms': round(build * 1e3, 3), 'trace_ms': round(statistics.median(ms), 4),
            'rays': int(rays_o.shape[0]), 'hit_fraction': round(float((t < 10).float().mean()), 5),
            'mean_hit_depth': round(float(t[t < 10].double().mean()), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--cell', type=float, default=2.0)
    ap.add_argument('--target-faces', type=int, default=100000)
    ap.add_argument('--rays', type=int, default=1 << 20)
    ap.add_argument('--bvh-build', choices=('host', 'device'), default='host', help='where trace_cost builds the tracer\'s tree')
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is none'
    from bench_mesh import model
    from nero_amd import mesh as M
    dev = torch.device('cuda:0')
    net = model(dev)
    net.extract_geometry(resolution=64, simplify={'cell': 2.0})          # warm-up (packing, allocator, code objects)
    out = {'metric': 'stage1_mesh_simplify', 'device': torch.cuda.get_device_name(0), 'hbm_TBps_achievable': HBM_TBS}
    g = torch.Generator(device=dev).manual_seed(6033)
    d = torch.randn((args.rays, 3), generator=g, device=dev)
    rays_o = 1.5 * d / d.norm(dim=1, keepdim=True)
    target = torch.randn((args.rays, 3), generator=g, device=dev)
    target = target / target.norm(dim=1, keepdim=True) * torch.rand((args.rays, 1), generator=g, device=dev) ** (1 / 3)
    rays_d = target - rays_o
    rays_d = rays_d / rays_d.norm(dim=1, keepdim=True)
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        row = {'V': int(verts.shape[0]), 'T': int(tris.shape[0])}
        d_cell, (v2, f2, info) = wall_median(lambda: M.simplify_mesh_device(verts, tris, cell=args.cell), args.reps)
        r = kernels(verts, tris, args.cell, args.reps)
        d_host, (vh, fh) = wall_median(lambda: host_route(verts, tris, args.cell), args.host_reps)
        assert torch.equal(f2, fh) and r['T_out'] == len(f2)                # both routes give the same faces
        r.update(simplify_mesh_device_ms=round(d_cell * 1e3, 4), numpy_restatement_ms=round(d_host * 1e3, 2),
                 max_abs_diff_vs_numpy=float((v2 - vh).abs().max()))
        row[f'cell_{args.cell:g}'] = r
        d_budget, (vb, fb, info_b) = wall_median(lambda: M.simplify_mesh_device(verts, tris, target_faces=args.target_faces), args.reps)
        rb = kernels(verts, tris, info_b.cell, args.reps)
        rb.update(k=info_b.k, simplify_mesh_device_ms=round(d_budget * 1e3, 4), n_duplicates=info_b.n_duplicates)
        row[f'target_{args.target_faces}'] = rb
        row['trace'] = {'original': trace_cost(verts, tris, res, rays_o, rays_d, 5, args.bvh_build),
                        f'cell_{args.cell:g}': trace_cost(v2, f2, res, rays_o, rays_d, 5, args.bvh_build),
                        f'target_{args.target_faces}': trace_cost(vb, fb, res, rays_o, rays_d, 5, args.bvh_build)}
        out[f'{res}^3'] = row
        del verts, tris, v2, f2, vb, fb
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_mesh_simplify.json'), 'w') as fh_:
            fh_.write(line + '\n')


if __name__ == '__main__':
    main()
