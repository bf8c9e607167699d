"""Exact point-to-mesh distance on one MI355X (RayTracer.closest / nero_bvh_closest, nero_amd/eval_shape.py: point_to_mesh): --n surface
samples of one marching-cubes mesh of the model bench.py's inference_bench uses (scripts/bench_mesh.py) against the mesh extracted at the
other resolution, for each of --res.  Per mesh:
  * the call alone (HIP events), queries in the order the sampler gives them and in Morton order (sorted once, outside the timing);
  * the whole point_to_mesh from device tensors and a ready tracer (wall clock), with sort=False and sort=True (the sort inside the timing);
  * beside it nearest_dist on the same --n + --n samples (what eval_meshes(exact=False) computes per direction), and a plain-torch brute force
    over all triangles (the same four-candidate arithmetic, tests/closest_ref.py's, written with torch) on --brute queries, a size it can hold.
The sides ALTERNATE, --reps rounds after one warm-up round; every figure is the median with [min, max].  Prints one JSON line and writes it
to profiles/bench_closest_point.json.  Nothing is asserted about the times.

    python scripts/bench_closest_point.py [--res 256 512] [--n 500000] [--brute 256] [--reps 7] [--no-write]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def spread(xs):
    return {'median': round(statistics.median(xs), 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4)}


def torch_brute_force(pts, verts, tris, rows=64):
    """distance from every point to the nearest triangle, over ALL triangles, `rows` points at a time: the three edge segments and the
    clamped foot of the perpendicular, as closest_point_math.h has them, in plain torch"""
    v0 = verts[tris[:, 0].long()]
    e1, e2 = verts[tris[:, 1].long()] - v0, verts[tris[:, 2].long()] - v0
    dot = lambda a, b: (a * b).sum(-1)

    def seg(w, e):
        l2 = dot(e, e)
        return torch.where(l2 > 0, (dot(w, e) / l2.clamp_min(1e-38)).clamp(0, 1), torch.zeros_like(l2))

    def d2_of(d, b1, b2):
        r = d - (b1[..., None] * e1 + b2[..., None] * e2)
        return dot(r, r)
    n = torch.cross(e1, e2, dim=-1)
    nn = dot(n, n)
    out = []
    for lo in range(0, pts.shape[0], rows):
        d = pts[lo:lo + rows, None, :] - v0[None]
        z = torch.zeros_like(d[..., 0])
        best = torch.minimum(d2_of(d, seg(d, e1), z), d2_of(d, z, seg(d, e2)))
        t = seg(d - e1, e2 - e1)
        best = torch.minimum(best, d2_of(d, 1 - t, t))
        b1 = (dot(torch.cross(d, e2.expand_as(d), dim=-1), n) / nn.clamp_min(1e-38)).clamp(0, 1)
        b2 = torch.minimum((dot(torch.cross(e1.expand_as(d), d, dim=-1), n) / nn.clamp_min(1e-38)).clamp_min(0), 1 - b1)
        best = torch.where(nn > 0, torch.minimum(best, d2_of(d, b1, b2)), best)
        out.append(best.min(1).values.sqrt())
    return torch.cat(out)


def measure(verts, tris, queries, own_samples, n_brute, reps, bvh_build):
    from nero_amd import eval_shape as E
    from nero_amd.raytracing import RayTracer, _morton30
    rt = RayTracer(verts, tris, build=bvh_build)
    info = rt.info()
    n = queries.shape[0]
    sorted_q = queries[torch.sort(_morton30(queries), stable=True)[1]].contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    rows = {k: [] for k in ('call_unsorted_ms', 'call_sorted_ms', 'point_to_mesh_ms', 'point_to_mesh_sorting_ms', 'nearest_dist_ms', 'torch_brute_ms')}
    worst = 0.0
    for it in range(reps + 1):                                         # (round 0: code objects, the tree, the allocator)
        ev[0].record()
        a = rt.closest(queries)[0]
        ev[1].record()
        b = rt.closest(sorted_q)[0]
        ev[2].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = E.point_to_mesh(queries, rt, sort=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d = E.point_to_mesh(queries, rt, sort=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        nd = E.nearest_dist(queries, own_samples)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        bf = torch_brute_force(queries[:n_brute], verts, tris)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        assert torch.equal(a, c) and torch.equal(a, d) and torch.equal(a.sort()[0], b.sort()[0])
        worst = max(worst, float((bf - a[:n_brute]).abs().max()))
        if it >= 1:
            rows['call_unsorted_ms'].append(ev[0].elapsed_time(ev[1]))
            rows['call_sorted_ms'].append(ev[1].elapsed_time(ev[2]))
            rows['point_to_mesh_ms'].append((t1 - t0) * 1e3)
            rows['point_to_mesh_sorting_ms'].append((t2 - t1) * 1e3)
            rows['nearest_dist_ms'].append((t3 - t2) * 1e3)
            rows['torch_brute_ms'].append((t4 - t3) * 1e3)
    out = {'V': int(verts.shape[0]), 'T': int(tris.shape[0]), 'n': n, 'n_brute': n_brute, 'reps': reps, 'tree': info,
           'mean_dist': float(a.mean()), 'mean_nearest_sample_dist': float(nd.mean()), 'max_abs_diff_to_torch_brute': worst}
    out.update({k: spread(x) for k, x in rows.items()})
    out['brute_ms_per_query_over_call_ms_per_query'] = round((out['torch_brute_ms']['median'] / n_brute) / (out['call_sorted_ms']['median'] / n), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--n', type=int, default=500000)
    ap.add_argument('--brute', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--bvh-build', choices=('host', 'device'), default='device')
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    from bench_mesh import model
    from nero_amd import mesh as M
    from nero_amd.surface import sample_surface
    dev = torch.device('cuda:0')
    net = model(dev)
    meshes, clouds = {}, {}
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        meshes[res] = ((verts / (res - 1.0) * 2.0 - 1.0).contiguous(), tris)       # grid indices -> the unit-scale world the query is padded for
        clouds[res] = sample_surface(*meshes[res], args.n, seed=0)
    out = {'metric': 'closest_point', 'device': torch.cuda.get_device_name(0), 'bvh_build': args.bvh_build}
    for k, res in enumerate(args.res):
        other = args.res[(k + 1) % len(args.res)]
        out[f'{other}^3_samples_to_{res}^3_mesh'] = measure(*meshes[res], clouds[other], clouds[res], min(args.brute, args.n), args.reps,
                                                          args.bvh_build)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_closest_point.json'), 'w') as fh_:
            fh_.write(line + '\n')


if __name__ == '__main__':
    main()
