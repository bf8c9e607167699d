"""The chart atlas (nero_amd/csrc/mesh_atlas.hip, nero_amd.texture.chart_atlas) on one MI355X: face adjacency, chart labels + statistics,
the UV vertices (corners), the UV emission and the overlap count with HIP events (median over --reps after a warm-up), the host packing
(choose_scale) and the whole chart_atlas call with a host clock round work that ends in a synchronise (the call holds the read-backs),
on the cleaned marching-cubes mesh (keep the largest component) of the model bench.py's inference_bench, scripts/bench_mesh.py and
scripts/bench_mesh_clean.py use (seed 6033, perturb_state at variance 0.5).  Beside them the numpy restatement tests/mesh_atlas_ref.atlas
on the host of the same box in the same run, copies of the mesh included; both routes must give the same atlas, bit for bit.  The
expectation checked here, not tuned for: the device route is not slower than the host route at either size.  Prints one JSON line and
writes it to profiles/bench_atlas.json.

    python scripts/bench_atlas.py [--res 256 512] [--size 2048] [--reps 20] [--host-reps 1] [--out FILE]

Bytes of the kernels, from the shapes (V vertices, T triangles, n UV vertices, K charts): adjacency reads tris three times over (36 T),
writes and sorts 3T keys of 8 and values of 4 bytes (36 T to write, 72 T per radix pass; the pass count depends on V and is not
modelled: one pass), reads them back and writes nbr (36 T + 12 T); charts read tris and three vertices per face (12 T + 36 T), write class
and parent (8 T), read nbr and touch the parents of three neighbours (12 T + 12 T), flatten and number (16 T), and for the statistics read
tris, chart, class and three vertices again (56 T); corners write, sort and read 3T keys and values as adjacency does (36 T + 72 T + 36 T),
flag and scan (24 T) and write ft and the two vt arrays (12 T + 8 n); uv reads 8 n + 12 n and writes 8 n."""
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
HBM_TBS = 6.3          # achievable HBM rate of one MI355X (measuring guide), TB/s


def byte_model(V, T, n):
    adjacency = 36 * T + 36 * T + 72 * T + 48 * T
    charts = 48 * T + 8 * T + 24 * T + 16 * T + 56 * T
    corners = 36 * T + 72 * T + 36 * T + 24 * T + 12 * T + 8 * n
    uv = 28 * n
    return {'adjacency': adjacency, 'charts': charts, 'corners': corners, 'uv': uv, 'total': adjacency + charts + corners + uv}


def stages(verts, tris, size, gutter, reps):
    """the steps of chart_atlas one by one -> dict of medians (ms)"""
    from nero_amd import mesh as M
    from nero_amd import texture as TX
    V, T = verts.shape[0], tris.shape[0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
    rows, host = [], []
    for it in range(reps + 3):
        ev[0].record()
        nbr, nb, nm = M.face_adjacency_device(tris, V)
        ev[1].record()
        ev[2].record()
        chart, cls, _, ci = M.face_charts_device(verts, tris)           # (adjacency again inside: subtracted below)
        ev[3].record()
        ev[4].record()
        ft, vv, vc = TX.chart_corners_device(tris, V, chart, ci.K)
        ev[5].record()
        box = ci.box.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scale, rects, steps = TX.choose_scale(box, size, gutter)
        t_pack = time.perf_counter() - t0
        ev[6].record()
        vt = TX.chart_uv_device(verts, vv, vc, ci.chart_class, ci.box, rects, scale, size)
        ev[7].record()
        ev[8].record()
        over = TX.uv_overlap(vt, ft, size, size)
        ev[9].record()
        torch.cuda.synchronize()
        if it >= 3:                                                    # (warm-up: code objects, allocator)
            rows.append([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(5)])
            host.append(t_pack * 1e3)
    med = [statistics.median(r[i] for r in rows) for i in range(5)]
    nbytes = byte_model(V, T, vt.shape[0])
    kern = med[0] + (med[1] - med[0]) + med[2] + med[3]
    return {'V': V, 'T': T, 'charts': ci.K, 'chartless_faces': ci.n_chartless, 'boundary_edges': nb, 'nonmanifold_edges': nm, 'uv_vertices': int(vt.shape[0]),
            'size': size, 'gutter': gutter, 'scale_texels_per_unit': scale, 'bisection_steps': steps,
            'fill': round(float((rects[:, 2] * rects[:, 3]).sum()) / float(size * size), 4), 'overlap_texels': over, 'reps': reps,
            'adjacency_ms': round(med[0], 4), 'charts_ms': round(med[1] - med[0], 4), 'corners_ms': round(med[2], 4),
            'packing_host_ms': round(statistics.median(host), 4), 'uv_ms': round(med[3], 4), 'overlap_count_ms': round(med[4], 4),
            'bytes': nbytes, 'GBps_adjacency_to_uv': round(nbytes['total'] / (kern * 1e-3) / 1e9, 1),
            'frac_of_hbm': round(nbytes['total'] / (kern * 1e-3) / (HBM_TBS * 1e12), 4),
            'note': 'adjacency / charts / corners include their count read-backs; charts_ms = face_charts_device less the adjacency inside it'}


def wall_median(fn, reps):
    out = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if it >= 1 or reps == 0:
            out.append(time.perf_counter() - t0)
    return statistics.median(out), r


def host_route(verts, tris, size, gutter):
    """the mesh to the host, the numpy restatement, vt and ft back to the device"""
    from tests import mesh_atlas_ref as A
    r = A.atlas(verts.cpu().numpy(), tris.cpu().numpy(), size, gutter)
    return torch.from_numpy(r['vt']).to(verts.device), torch.from_numpy(r['ft']).to(verts.device), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--gutter', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_atlas.json'))
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    from bench_mesh import model
    from nero_amd import mesh as M
    from nero_amd import texture as TX
    dev = torch.device('cuda:0')
    net = model(dev)
    out = {'metric': 'stage2_chart_atlas', 'device': torch.cuda.get_device_name(0), 'hbm_TBps_achievable': HBM_TBS}
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        verts, tris, _ = M.clean_mesh_device(verts, tris, keep='largest')
        r = stages(verts, tris, args.size, args.gutter, args.reps)
        d_dev, (vt, ft, info) = wall_median(lambda: TX.chart_atlas(verts, tris, args.size, args.gutter), args.reps)
        d_host, (vth, fth, ref) = wall_median(lambda: host_route(verts, tris, args.size, args.gutter), args.host_reps - 1)
        same = bool(torch.equal(vt.view(torch.int32), vth.view(torch.int32)) and torch.equal(ft, fth) and info.scale == ref['scale']
                    and np.array_equal(info.rects, ref['rects']))
        assert same, 'the device atlas differs from the restatement'
        r.update(chart_atlas_ms=round(d_dev * 1e3, 4), host_restatement_ms=round(d_host * 1e3, 4), host_reps=max(1, args.host_reps),
                 device_not_slower_than_host=bool(d_dev <= d_host), host_over_device=round(d_host / d_dev, 1), same_atlas_bit_for_bit=same)
        out[f'{res}^3'] = r
        del verts, tris, vt, ft, vth, fth
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
