"""The ray tracer's BVH build on one MI355X, host builder against device build, same box, same meshes, same run: the wall time of the first
trace() on a fresh RayTracer (build + 64 rays, what bench_mesh_simplify.py's trace_cost calls bvh_build_ms; the mesh starts on the device,
so build='host' pays the copy to the host, the single-threaded C++ build and the upload), the device build's time by phase (HIP events on
the build's stream: prep, wide levels, finishing kernel, emit), and the trace of the fixed 1 M-ray set of bench_mesh_simplify.py through both
handles -- the same kernels on the same node bytes, with the host handle timed twice to show the run-to-run spread.  Meshes: icosphere(7,
0.5, 0.2), the marching-cubes mesh of the model scripts/bench_mesh.py uses at 256^3 and 512^3, and the 512^3 mesh simplified to 100 000
faces.  Prints one JSON line and writes it to profiles/bench_bvh_build.json.

    python scripts/bench_bvh_build.py [--res 256 512] [--reps 5] [--rays 1048576] [--no-write]"""
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


def first_trace(verts, tris, build, rays_o, rays_d, reps):
    """-> (median wall ms of RayTracer(...) + the first 64-ray trace, all samples, the tracer of the last repetition, phase ms or None)"""
    from nero_amd import _lib as L
    from nero_amd.raytracing import RayTracer
    ms, phases, tracer = [], [], None
    for _ in range(reps):
        del tracer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracer = RayTracer(verts, tris, build=build)
        tracer.trace(rays_o[:64], rays_d[:64])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if build == 'device':
            ph = (C.c_float * 4)()
            L.check(L.lib.nero_bvh_build_last_phase_ms(ph))
            phases.append(list(ph))
    ph = None
    if phases:
        ph = {k: round(statistics.median(p[i] for p in phases), 4) for i, k in enumerate(('prep_ms', 'wide_levels_ms', 'finish_ms', 'emit_ms'))}
        ph['sum_ms'] = round(sum(ph.values()), 4)
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms], tracer, ph


def trace_ms(tracer, rays_o, rays_d, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for it in range(reps + 2):
        ev[0].record()
        _, _, t = tracer.trace(rays_o, rays_d)
        ev[1].record()
        torch.cuda.synchronize()
        if it >= 2:
            out.append(ev[0].elapsed_time(ev[1]))
    return round(statistics.median(out), 4), t.reshape(-1)


def measure(verts, tris, rays_o, rays_d, reps):
    host_ms, host_all, host, _ = first_trace(verts, tris, 'host', rays_o, rays_d, reps)
    dev_ms, dev_all, dev, phases = first_trace(verts, tris, 'device', rays_o, rays_d, reps)
    info = dev.info()
    assert info == host.info()
    t_host_a, th = trace_ms(host, rays_o, rays_d, reps)
    t_dev, td = trace_ms(dev, rays_o, rays_d, reps)
    t_host_b, _ = trace_ms(host, rays_o, rays_d, reps)
    assert torch.equal(th, td)                                         # the same tree: the same depths
    return {'V': int(verts.shape[0]), 'T': int(tris.shape[0]), **info, 'reps': reps,
            'first_trace_host_ms': host_ms, 'first_trace_host_samples': host_all,
            'first_trace_device_ms': dev_ms, 'first_trace_device_samples': dev_all,
            'host_over_device': round(host_ms / dev_ms, 2), 'device_build_phases': phases,
            'trace_ms_host_handle': t_host_a, 'trace_ms_device_handle': t_dev, 'trace_ms_host_handle_again': t_host_b,
            'rays': int(rays_o.shape[0]), 'hit_fraction': round(float((th < 10).float().mean()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--target-faces', type=int, default=100000)
    ap.add_argument('--rays', type=int, default=1 << 20)
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is none'
    from bench_mesh import model
    from nero_amd import _lib as L
    from nero_amd import mesh as M
    from nero_amd.synthetic import icosphere
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(6033)                  # the ray set of bench_mesh_simplify.py
    d = torch.randn((args.rays, 3), generator=g, device=dev)
    rays_o = 1.5 * d / d.norm(dim=1, keepdim=True)
    target = torch.randn((args.rays, 3), generator=g, device=dev)
    target = target / target.norm(dim=1, keepdim=True) * torch.rand((args.rays, 1), generator=g, device=dev) ** (1 / 3)
    rays_d = target - rays_o
    rays_d = rays_d / rays_d.norm(dim=1, keepdim=True)
    out = {'metric': 'bvh_build', 'device': torch.cuda.get_device_name(0), 'lds_capacity': int(L.lib.nero_bvh_build_lds_capacity())}
    v, f = icosphere(3, 0.5, 0.2)                                      # warm-up: code objects, allocator, both builders
    measure(torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev), rays_o[:4096], rays_d[:4096], 1)
    v, f = icosphere(7, 0.5, 0.2)
    out['icosphere_7'] = measure(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev), rays_o, rays_d, args.reps)
    net = model(dev)
    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        world = (verts / (res - 1.0) * 2.0 - 1.0).contiguous()
        out[f'{res}^3'] = measure(world, tris, rays_o, rays_d, args.reps)
        if res == max(args.res):
            vb, fb, _ = M.simplify_mesh_device(verts, tris, target_faces=args.target_faces)
            out[f'{res}^3_target_{args.target_faces}'] = measure((vb / (res - 1.0) * 2.0 - 1.0).contiguous(), fb, rays_o, rays_d, args.reps)
        del verts, tris, world
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_bvh_build.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
