"""Shadow rays and ambient occlusion on one MI355X, each comparison alternated in one process on the same inputs (HIP events, median
over --reps after a warm-up):
  * nero_bvh_occluded (any hit) against nero_bvh_trace (closest hit) on 1 M secondary rays leaving the surface and on 1 M camera rays, at
    tmax = 10 (the miss distance) and a short tmax, on the marching-cubes meshes scripts/bench_bvh_build.py uses (256^3: ~90 k triangles,
    512^3: ~360 k);
  * nero_bvh_ao (rays made and cast in one kernel) against the unfused route -- nero_ao_rays, nero_bvh_occluded, a torch sum -- at 64
    samples on 16 384 surface points (1 M rays), with the 24 bytes per ray the fused call does not move turned into an ESTIMATED time at an
    assumed HBM rate; medians with their minimum and maximum;
  * the whole bake_ambient_occlusion (chart atlas given, 64 samples) at 1024 and 2048, ssaa 2, on the smaller mesh: wall time, the minimum of
    two runs after one warm-up run, all three samples listed.
Prints one JSON line and writes it to profiles/bench_ao.json.

    python scripts/bench_ao.py [--res 256 512] [--reps 7] [--sizes 1024 2048] [--no-write]"""
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
HBM_TBS = 6.3          # ASSUMED achievable HBM rate of one MI355X, TB/s: turns the unmoved bytes into an estimate, nothing here measures it


def alternate(fns, reps, warmup=2, spread=False):
    """the callables of `fns` in turn, reps + warmup rounds -> median ms of each (HIP events); spread: (median, min, max) of each"""
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
    if spread:
        return [(round(statistics.median(m), 4), round(min(m), 4), round(max(m), 4)) for m in ms]
    return [round(statistics.median(m), 4) for m in ms]


def ray_pair(rt, o, d, tmax, reps):
    from nero_amd import _lib as L
    n = o.shape[0]
    pos, nrm, depth = torch.empty_like(o), torch.empty_like(o), torch.empty(n, device=o.device)
    occ = torch.empty(n, dtype=torch.uint8, device=o.device)
    h, s = rt._handle(), L.stream_ptr()
    trace = lambda: L.check(L.lib.nero_bvh_trace(h, o.data_ptr(), d.data_ptr(), n, pos.data_ptr(), nrm.data_ptr(), depth.data_ptr(), s))
    out = {}
    for t in tmax:
        anyhit = lambda: L.check(L.lib.nero_bvh_occluded(h, o.data_ptr(), d.data_ptr(), n, None, t, None, occ.data_ptr(), s))
        (a, a0, a1), (b, b0, b1) = alternate([trace, anyhit], reps, spread=True)
        agree = float((occ.bool() == (depth < t)).float().mean())
        out[f'tmax_{t:g}'] = {'trace_ms': a, 'occluded_ms': b, 'trace_ms_min_max': [a0, a1], 'occluded_ms_min_max': [b0, b1],
                              'occluded_over_trace': round(b / a, 4),
                              'occluded_share': round(float(occ.float().mean()), 5), 'agreement_with_depth_lt_tmax': agree}
    return out


def surface_points(v, f, P, seed):
    """P face centroids with unit normals pointing away from the inside (decided per mesh by which side sees less occlusion)"""
    g = torch.Generator(device=v.device).manual_seed(seed)
    ti = torch.randint(0, f.shape[0], (P,), generator=g, device=v.device)
    tri = v[f[ti].long()]
    n = torch.nn.functional.normalize(torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), dim=-1)
    return tri.mean(1).contiguous(), n.contiguous(), ti.int().contiguous()


def measure_mesh(v, f, reps, sizes):
    from nero_amd import _lib as L
    from nero_amd import texture as TX
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import camera_rays
    dev = v.device
    rt = RayTracer(v, f, build='device')
    out = {'V': int(v.shape[0]), 'T': int(f.shape[0]), **rt.info()}
    S, P = 64, 16384
    pts, nrm, key = surface_points(v, f, P, 1)
    c_out = TX.ambient_occlusion(rt, pts, nrm, key, samples=S)
    c_in = TX.ambient_occlusion(rt, pts, -nrm, key, samples=S)
    flip = bool(c_in.sum() < c_out.sum())                              # the winding of the mesh: outward is the side that sees less
    if flip:
        nrm = (-nrm).contiguous()
    out['normals_flipped'] = flip
    # 1 M secondary rays: the AO sample set itself (cosine-distributed, leaving the surface), and 1 M camera rays
    o = torch.empty((P * S, 3), device=dev)
    d = torch.empty((P * S, 3), device=dev)
    s = L.stream_ptr()
    L.check(L.lib.nero_ao_rays(pts.data_ptr(), nrm.data_ptr(), key.data_ptr(), P, S, 0, 1e-4, o.data_ptr(), d.data_ptr(), s))
    out['secondary_1M'] = ray_pair(rt, o, d, (10.0, 0.2), reps)
    co, cd = camera_rays(1024, device=dev)
    out['camera_1M'] = ray_pair(rt, co, cd, (10.0, 1.7), reps)
    # fused against unfused
    count = torch.empty(P, dtype=torch.int32, device=dev)
    occ = torch.empty(P * S, dtype=torch.uint8, device=dev)
    h = rt._handle()
    res = {}

    def fused():
        L.check(L.lib.nero_bvh_ao(h, pts.data_ptr(), nrm.data_ptr(), key.data_ptr(), P, S, 0, 1e-4, 10.0, count.data_ptr(), s))

    def unfused():
        L.check(L.lib.nero_ao_rays(pts.data_ptr(), nrm.data_ptr(), key.data_ptr(), P, S, 0, 1e-4, o.data_ptr(), d.data_ptr(), s))
        L.check(L.lib.nero_bvh_occluded(h, o.data_ptr(), d.data_ptr(), P * S, None, 10.0, None, occ.data_ptr(), s))
        res['count'] = occ.view(P, S).sum(1, dtype=torch.int32)
    (a, a0, a1), (b, b0, b1) = alternate([fused, unfused], reps, spread=True)
    assert torch.equal(count, res['count'])
    moved_ms = 24.0 * P * S / (HBM_TBS * 1e12) * 1e3                     # 12 bytes of origin and 12 of direction per ray, written once
    out['ao_64_samples_1M_rays'] = {'fused_ms': a, 'unfused_ms': b, 'fused_ms_min_max': [a0, a1], 'unfused_ms_min_max': [b0, b1],
                                    'unfused_minus_fused_ms': round(b - a, 4), 'assumed_hbm_tb_per_s': HBM_TBS,
                                    'estimated_ms_of_24_bytes_per_ray': round(moved_ms, 4), 'estimated_ms_if_also_read_back': round(2 * moved_ms, 4),
                                    'mean_occlusion': round(float(count.float().mean()) / S, 5)}
    if sizes:
        out['bake'] = {}
        for size in sizes:
            try:
                vt, ft, info = TX.chart_atlas(v, f, size)
            except ValueError as e:                                    # the charts of this mesh do not fit a map of this size
                out['bake'][str(size)] = {'error': str(e)}
                continue
            ms = []
            for it in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                baked = TX.bake_ambient_occlusion(v, f, vt=vt, ft=ft, size=size, ssaa=2, samples=S, flip_normals=flip, tracer=rt,
                                                  return_intermediates=True)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            n_tex = int(baked['texel'].shape[0])
            ao_only = alternate([lambda: TX.ambient_occlusion(rt, baked['points'], baked['normals'], baked['texel'], samples=S)], 3, 1)[0]
            out['bake'][str(size)] = {'wall_ms_min': round(min(ms[1:]), 3), 'wall_ms_samples': [round(x, 3) for x in ms], 'covered_texels': n_tex,
                                      'rays': n_tex * S, 'ao_kernel_ms': ao_only, 'grays_per_s': round(n_tex * S / ao_only / 1e6, 3),
                                      'charts': info.n_charts, 'mean_level': round(float(baked['ao'][baked['mask']].float().mean()), 3)}
            del baked
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[1024, 2048])
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is none'
    from bench_mesh import model
    from nero_amd import mesh as M
    from nero_amd.synthetic import icosphere
    dev = torch.device('cuda:0')
    out = {'metric': 'ao', 'device': torch.cuda.get_device_name(0), 'samples': 64}
    v, f = icosphere(3, 0.5, 0.2)                                      # warm-up: code objects, allocator
    measure_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev), 1, [])
    net = model(dev)
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        world = (verts / (res - 1.0) * 2.0 - 1.0).contiguous()
        out[f'{res}^3'] = measure_mesh(world, tris, args.reps, args.sizes if res == min(args.res) else [])
        del verts, tris, world
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_ao.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
