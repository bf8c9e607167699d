"""The texture lookup on one MI355X (include/nero_hip_texfetch.h, nero_amd/texfetch.py).  Everything that is compared is
alternated in one process on the same inputs (HIP events around 20 calls, per call; median over --reps after a warm-up, with minimum
and maximum):
  * pack plus pyramid (nero_tex_pack, nero_tex_mip_build) of random maps at 1024^2 and 2048^2, with the rate of the BYTE MODEL: 5 bytes
    read and 8 written per texel of level 0, and per record of a level above it 32 read and 8 written;
  * the fused fetch (nero_tex_materials) of --hits hits spread over the bench mesh of bench_relight.py (a bumpy icosphere of 81 920
    triangles under a simple_atlas at 2048^2), at level 0 alone (spread 0) and at footprints that span the pyramid, against the same
    arithmetic in plain torch on the same GPU (gathers of the records, the table and the three mixes), with the distance between the two.
    BYTE MODEL of a hit: 16 of face, barycentrics and depth, 40 of the face's UV indices, UVs and scale, 8 per tap (4 taps where t = 0,
    else 8), 20 written: what the lanes ask for, not what reaches HBM -- neighbouring hits ask for the same texels;
  * Relighter.surface() of an 800 x 800 view of that mesh, textured against per-vertex, and the trace alone.
Prints one JSON line and writes it to profiles/bench_tex_fetch.json.

    python scripts/bench_tex_fetch.py [--reps 9] [--hits 1000000] [--no-write]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


INNER = 20          # calls per timed window: one call is a tenth of a millisecond, too short a window for an event pair


def alternate(fns, reps, warmup=3):
    """the callables of `fns` in turn, reps + warmup rounds of INNER calls each -> (median, min, max) ms per call of each (HIP events)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = [[] for _ in fns]
    for it in range(reps + warmup):
        for k, fn in enumerate(fns):
            ev[0].record()
            for _ in range(INNER):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(ev[0].elapsed_time(ev[1]) / INNER)
    return [(round(statistics.median(m), 4), round(min(m), 4), round(max(m), 4)) for m in ms]


def torch_fetch(tex, vt, ft, scale, face, bary, depth, spread, lod_scale):
    """nero_tex_materials in plain torch (finite inputs, faces in range) -> mat5 [n,5]"""
    L = tex.levels
    dev = tex.device
    rec = tex.pyramid.view(-1, 8)
    H = torch.tensor([tex.h >> k for k in range(L)], device=dev)
    W = torch.tensor([tex.w >> k for k in range(L)], device=dev)
    off = torch.cumsum(H * W, 0) - H * W
    f = face.long()
    j = ft[f].long()
    bu, bv = bary[:, 0:1], bary[:, 1:2]
    uv = (((1.0 - bu) - bv) * vt[j[:, 0]] + bu * vt[j[:, 1]]) + bv * vt[j[:, 2]]
    s = torch.clamp(((depth * spread) * scale[f]) * lod_scale, min=1.0)
    l = torch.clamp(torch.frexp(s)[1].long() - 1, max=L - 1)
    t = torch.where(l < L - 1, s * torch.exp2(-l.float()) - 1.0, torch.zeros_like(s))

    def bilinear(k):
        wk, hk = W[k], H[k]

        def axis(c, n):
            x = torch.minimum(torch.clamp(c * n - 0.5, min=-1.0), n.float())
            x0 = torch.floor(x)
            i0 = x0.long()
            return torch.minimum(torch.clamp(i0, min=0), n - 1), torch.minimum(torch.clamp(i0 + 1, min=0), n - 1), (x - x0)[:, None]
        xa, xb, fx = axis(uv[:, 0], wk)
        ya, yb, fy = axis(uv[:, 1], hk)
        dec = lambda yy, xx: tex.lut[rec[off[k] + yy * wk + xx][:, :5].long()]
        p00, p01, p10, p11 = dec(ya, xa), dec(ya, xb), dec(yb, xa), dec(yb, xb)
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        return top + fy * (bot - top)
    lo = bilinear(l)
    val = lo + t[:, None] * (bilinear(torch.clamp(l + 1, max=L - 1)) - lo)
    return torch.cat([val[:, 3:4], torch.sqrt(val[:, 4:5]), val[:, 0:3]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--hits', type=int, default=1000000)
    ap.add_argument('--no-write', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib as L
    from nero_amd import relight as RL
    from nero_amd import texfetch as TF
    from nero_amd.synthetic import icosphere
    from nero_amd.texture import simple_atlas
    assert torch.cuda.is_available(), 'bench_tex_fetch.py measures on a GPU'
    g = np.random.default_rng(0)
    out = {'reps': a.reps, 'calls_per_timed_window': INNER, 'device': torch.cuda.get_device_name(0),
           'byte_model': 'pack: 5 read + 8 written per texel; a level above: 32 read + 8 written per record; a hit: 56 of inputs + 8 per tap '
                         '(4 taps where t = 0, else 8) + 20 written: what the lanes ask for, not HBM traffic'}
    # ---- pack plus pyramid ------------------------------------------------------------------------------------------------------------
    maps = {}
    for n in (1024, 2048):
        m = [torch.from_numpy(g.integers(0, 256, shape, dtype=np.uint8)).cuda() for shape in ((n, n, 3), (n, n), (n, n))]
        maps[n] = m
        pyr = torch.empty(int(L.lib.nero_tex_mip_bytes(n, n)), dtype=torch.uint8, device='cuda')

        def build(m=m, n=n, pyr=pyr):
            L.check(L.lib.nero_tex_pack(L.ptr(m[0]), L.ptr(m[1]), L.ptr(m[2]), n, n, L.ptr(pyr), L.stream_ptr()))
            L.check(L.lib.nero_tex_mip_build(L.ptr(pyr), n, n, L.stream_ptr()))
        (med, lo, hi), = alternate([build], a.reps)
        above = pyr.numel() // 8 - n * n
        model = 13 * n * n + 40 * above
        out[f'pack_and_pyramid_{n}'] = {'ms': med, 'ms_min_max': [lo, hi], 'levels': TF.mip_levels(n, n), 'launches': TF.mip_levels(n, n),
                                        'model_bytes': model, 'model_GB_per_s': round(model / med / 1e6, 1)}
    # ---- the fetch --------------------------------------------------------------------------------------------------------------------
    v, f = icosphere(6, 0.5, 0.15)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
    vt, ft = simple_atlas(v, f, 2048)
    tex = TF.TextureSet(*maps[2048])
    vt_d, ft_d = torch.from_numpy(vt).cuda(), torch.from_numpy(ft).cuda()
    scale = TF.face_scale(v, f, vt, ft, 2048, 2048)
    n = a.hits
    face = torch.from_numpy(g.integers(0, len(f), n).astype(np.int32)).cuda()
    bary = g.uniform(0, 1, (n, 2)).astype(np.float32)
    bary[:, 1] *= 1 - bary[:, 0]
    bary = torch.from_numpy(bary).cuda()
    res = {'hits': n, 'mesh_triangles': int(len(f)), 'map': 2048, 'median_texels_per_world_unit': float(scale.median())}
    # footprints: level 0 alone; what an 800 x 800 view of the mesh from 3 units has; log-uniform over the whole pyramid
    cases = {'level_0': (torch.ones(n, device='cuda'), 0.0),
             'view_800_from_3_units': (torch.from_numpy(g.uniform(2.4, 3.0, n).astype(np.float32)).cuda(), 1.0 / float(RL.default_K(800, 800)[0, 0])),
             'all_levels': (torch.exp2(torch.from_numpy(g.uniform(0, 12, n).astype(np.float32))).cuda() / float(scale.median()), 1.0)}
    for name, (depth, spread) in cases.items():
        ker = lambda: TF.fetch_materials(tex, vt_d, ft_d, scale, face, bary, depth, spread)
        ref = lambda: torch_fetch(tex, vt_d, ft_d, scale, face, bary, depth, spread, 1.0)
        (k_ms, r_ms) = alternate([ker, ref], a.reps)
        got, dbg = TF.fetch_materials(tex, vt_d, ft_d, scale, face, bary, depth, spread, return_debug=True)
        two = int((dbg[:, 1] != 0).sum())
        model = n * (56 + 20) + 8 * (4 * (n - two) + 8 * two)
        res[name] = {'kernel_ms': k_ms[0], 'kernel_ms_min_max': list(k_ms[1:]), 'torch_ms': r_ms[0], 'torch_ms_min_max': list(r_ms[1:]),
                     'torch_over_kernel': round(r_ms[0] / k_ms[0], 1), 'hits_between_two_levels': two,
                     'levels_seen': sorted(set(dbg[:, 0].int().tolist())), 'model_bytes': model, 'model_GB_per_s': round(model / k_ms[0] / 1e6, 1),
                     'max_abs_distance_torch_from_kernel': float((ref() - got).abs().max())}
    out['fetch'] = res
    # ---- surface() of a view ----------------------------------------------------------------------------------------------------------
    mats = {'metallic': g.uniform(0, 1, (len(v), 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (len(v), 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (len(v), 3)).astype(np.float32)}
    env = torch.from_numpy(g.uniform(0.2, 1.2, (64, 128, 3)).astype(np.float32))
    plain = RL.Relighter(v, f, mats, env)
    textured = RL.Relighter(v, f, None, env, tracer=plain.tracer,
                            textures={'albedo': maps[2048][0], 'metallic': maps[2048][1], 'roughness': maps[2048][2], 'vt': vt, 'ft': ft})
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(8, 0.0, 30.0, 3.0))[3]
    K = RL.default_K(800, 800)
    ro, rd = plain.camera_rays(pose, K, 800, 800)
    spread = 1.0 / float(K[0, 0])
    sf = textured.surface(ro, rd, spread=spread)
    depth_, face_, bary_ = RL.trace_faces(plain.tracer, ro, rd)
    idx = sf['idx']
    fd, fb, ff = depth_[idx].contiguous(), bary_[idx].contiguous(), face_[idx].contiguous()
    _, dbg = TF.fetch_materials(textured.textures, textured.vt, textured.ft, textured.face_scale, ff, fb, fd, spread, return_debug=True)
    names = ['surface_textured', 'surface_per_vertex', 'trace_alone', 'fetch_alone']
    fns = [lambda: textured.surface(ro, rd, spread=spread), lambda: plain.surface(ro, rd), lambda: RL.trace_faces(plain.tracer, ro, rd),
           lambda: TF.fetch_materials(textured.textures, textured.vt, textured.ft, textured.face_scale, ff, fb, fd, spread)]
    view = {'pixels': 800 * 800, 'hit_pixels': int(idx.numel()), 'levels_seen': sorted(set(dbg[:, 0].int().tolist())),
            'median_footprint_texels': float(torch.exp2(dbg[:, 0] + torch.log2(1.0 + dbg[:, 1])).median())}
    for name, (med, lo, hi) in zip(names, alternate(fns, a.reps)):
        view[name] = {'ms': med, 'ms_min_max': [lo, hi]}
    view['textured_over_per_vertex'] = round(view['surface_textured']['ms'] / view['surface_per_vertex']['ms'], 3)
    out['surface_800x800'] = view
    line = json.dumps(out)
    print(line)
    if not a.no_write:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'bench_tex_fetch.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
