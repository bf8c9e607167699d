"""Detail transfer on one MI355X (include/nero_transfer.h, nero_amd/transfer.py).  The dense mesh is a stand-in for a
model's: the bench mesh of the other scripts -- a bumpy icosphere, --subdiv 7: 327 680 triangles (8: 1.3 M, the size a 512^3
extraction gives) -- simplified to --target-faces 100 000 with simplify_mesh_device, under a chart atlas.  Medians over --reps after a
warm-up, with minimum and maximum (HIP events around whole calls, the host's share included):
  * uv_tangents of the simplified mesh; the closest query and nero_nmap_encode over the covered texels of a 2048^2 rasterisation;
  * the whole bake_normal_map at 1024 and 2048, ssaa 2; the whole bake_asset at 1024, ssaa 2, with a freshly initialised material network;
  * nero_nmap_apply per --hits hits at level 0 and between two levels, against the same arithmetic in plain torch on the same GPU, with
    the distance between the two (the torch version has no fallbacks: hits where the map tilts past a right angle are counted apart);
  * Relighter.surface() of an 800 x 800 view of the simplified mesh with and without the map.
Prints one JSON line and writes it to profiles/bench_transfer.json.

    python scripts/bench_transfer.py [--reps 5] [--hits 1000000] [--subdiv 7] [--target-faces 100000] [--no-write]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup=2, inner=1):
    """-> {'ms': median, 'ms_min_max': [min, max]} per call over reps windows of `inner` calls after `warmup` windows (HIP events; a call
    of a tenth of a millisecond is too short a window for an event pair: inner=20 there)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for it in range(reps + warmup):
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]) / inner)
    return {'ms': round(statistics.median(ms), 4), 'ms_min_max': [round(min(ms), 4), round(max(ms), 4)]}


def torch_apply(nm, vt, ft, scale, tangent, sign, face, bary, depth, nrm_in, spread):
    """nero_nmap_apply in plain torch (tangent space, finite inputs, faces in range, no fallbacks) -> [n,3]"""
    L, dev = nm.levels, nm.device
    rec = nm.pyramid.view(-1, 4)
    H = torch.tensor([nm.h >> k for k in range(L)], device=dev)
    W = torch.tensor([nm.w >> k for k in range(L)], device=dev)
    off = torch.cumsum(H * W, 0) - H * W
    f = face.long()
    j = ft[f].long()
    bu, bv = bary[:, 0:1], bary[:, 1:2]
    mix = lambda X: (((1.0 - bu) - bv) * X[j[:, 0]] + bu * X[j[:, 1]]) + bv * X[j[:, 2]]
    uv = mix(vt)
    s = torch.clamp((depth * spread) * scale[f], min=1.0)
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
        dec = lambda yy, xx: (rec[off[k] + yy * wk + xx][:, :3].float() - 128.0) / 127.0
        p00, p01, p10, p11 = dec(ya, xa), dec(ya, xb), dec(yb, xa), dec(yb, xb)
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        return top + fy * (bot - top)
    lo = bilinear(l)
    m = lo + t[:, None] * (bilinear(torch.clamp(l + 1, max=L - 1)) - lo)
    ln = nrm_in.norm(dim=1, keepdim=True)
    n = nrm_in / ln
    T = mix(tangent)
    p = T - (T * n).sum(1, keepdim=True) * n
    tt = p / p.norm(dim=1, keepdim=True)
    b = torch.where(sign[f][:, None] < 0, -1.0, 1.0) * torch.linalg.cross(n, tt)
    return ((m[:, 0:1] * tt + m[:, 1:2] * b) * ln) + m[:, 2:3] * nrm_in


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hits', type=int, default=1000000)
    ap.add_argument('--subdiv', type=int, default=7)
    ap.add_argument('--target-faces', type=int, default=100000)
    ap.add_argument('--no-write', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight as RL
    from nero_amd import texfetch, texture as TX, transfer as TF
    from nero_amd.mesh import simplify_mesh_device, vertex_normals
    from nero_amd.raytracing import RayTracer
    from nero_amd.renderer import NeROMaterialRenderer
    from nero_amd.surface import sample_surface
    from nero_amd.synthetic import icosphere
    assert torch.cuda.is_available(), 'bench_transfer.py measures on a GPU'
    g = np.random.default_rng(0)
    v, f = icosphere(a.subdiv, 0.5, 0.15)
    src_v, src_f = torch.from_numpy(np.asarray(v, np.float32)).cuda(), torch.from_numpy(np.asarray(f, np.int32)).cuda()
    low_v, low_f = simplify_mesh_device(src_v, src_f, target_faces=a.target_faces)[:2]
    low_f = low_f.to(torch.int32).contiguous()
    tracer = RayTracer(src_v, src_f, build='device')
    out = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'source_triangles': int(src_f.shape[0]), 'target_triangles': int(low_f.shape[0]),
           'mesh': f'icosphere({a.subdiv}, 0.5, bumps=0.15), simplified to at most {a.target_faces} faces; chart atlas'}
    # ---- the pieces, at 2048 x 2048 ---------------------------------------------------------------------------------------------------
    vt, ft, info = TX.chart_atlas(low_v, low_f, 1024)
    out['charts'] = int(info.n_charts)
    nrm_v = vertex_normals(low_v, low_f, weight='angle', orient='outward')
    tri_id = TX.rasterize_uv(vt, ft, 2048, 2048)
    pr = TF._project(tracer, src_v, src_f, tri_id, vt, ft, low_v, low_f, nrm_v, None, 'angle')
    n_tex = int(pr['texel'].shape[0])
    out['covered_texels_2048'] = n_tex
    out['uv_tangents'] = timed(lambda: TF.uv_tangents(low_v, low_f, vt, ft), a.reps, inner=20)
    out['closest_2048'] = {**timed(lambda: tracer.closest(pr['points']), a.reps, inner=5), 'queries': n_tex}
    out['closest_2048']['M_queries_per_s'] = round(n_tex / out['closest_2048']['ms'] / 1e3, 1)
    valid = pr['face'] >= 0
    tex = torch.zeros((2048, 2048, 3), dtype=torch.uint8, device='cuda')
    out['encode_2048'] = timed(lambda: TF.encode_normals(pr['frame_normals'], pr['tangents'], pr['sign'], pr['source_normals'], valid, pr['texel'], 2048,
                                                         2048, 'tangent', out=tex), a.reps, inner=20)
    # ---- the whole bakes --------------------------------------------------------------------------------------------------------------
    baked = {}
    for size in (1024, 2048):
        def bake(size=size):
            baked[size] = TF.bake_normal_map(low_v, low_f, tracer, size=size, ssaa=2, atlas='charts')
        out[f'bake_normal_map_{size}_ssaa2'] = timed(bake, a.reps, warmup=1)
        out[f'bake_normal_map_{size}_ssaa2'].update(unmatched=baked[size]['unmatched'], max_moved=round(baked[size]['max_moved'], 6))
    net = NeROMaterialRenderer({}, is_train=False, mesh=(src_v.cpu().numpy(), src_f.cpu().numpy())).cuda().eval()
    out['bake_asset_1024_ssaa2'] = timed(lambda: TF.bake_asset(net, verts=low_v, tris=low_f, size=1024, ssaa=2), a.reps, warmup=1)
    # ---- the lookup -------------------------------------------------------------------------------------------------------------------
    bk = baked[2048]
    nm = TF.NormalMap(bk['normal'])
    scale = texfetch.face_scale(low_v, low_f, bk['vt'], bk['ft'], 2048, 2048)
    tangent, sign = TF.uv_tangents(low_v, low_f, bk['vt'], bk['ft'])
    n = a.hits
    _, face, bary = sample_surface(low_v, low_f, n, seed=1, return_face=True, return_bary=True)
    nrm_in = TF.attributes_at(nrm_v, low_f, face, bary)
    med = float(scale[scale > 0].median())
    cases = {'level_0': (torch.ones(n, device='cuda'), None),
             'between_two_levels': (torch.from_numpy(g.uniform(2.2, 3.8, n).astype(np.float32)).cuda() / med, 1.0)}
    res = {'hits': n, 'map': 2048, 'median_texels_per_world_unit': med}
    for name, (depth, spread) in cases.items():
        ker = lambda: TF.apply_normal_map(nm, bk['vt'], bk['ft'], scale, tangent, sign, face, bary, depth, nrm_in, spread)
        ref = lambda: torch_apply(nm, bk['vt'], bk['ft'], scale, tangent, sign, face, bary, depth, nrm_in, 0.0 if spread is None else spread)
        k, r = timed(ker, a.reps, inner=20), timed(ref, a.reps, inner=5)
        got, dbg = TF.apply_normal_map(nm, bk['vt'], bk['ft'], scale, tangent, sign, face, bary, depth, nrm_in, spread, return_debug=True)
        gap = (ref() - got).abs().amax(1)          # (the torch version has none of the kernel's fallbacks: a hit it tilts past 90 degrees differs)
        res[name] = {'kernel': k, 'torch': r, 'torch_over_kernel': round(r['ms'] / k['ms'], 1), 'hits_between_two_levels': int((dbg[:, 1] != 0).sum()),
                     'levels_seen': sorted(set(dbg[:, 0].int().tolist())), 'median_abs_distance_torch_from_kernel': float(gap.median()), 'hits_where_torch_is_beyond_1e-4': int((gap > 1e-4).sum())}
    out['apply'] = res
    # ---- surface() of a view ----------------------------------------------------------------------------------------------------------
    V = low_v.shape[0]
    mats = {'metallic': g.uniform(0, 1, (V, 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (V, 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (V, 3)).astype(np.float32)}
    env = torch.from_numpy(g.uniform(0.2, 1.2, (64, 128, 3)).astype(np.float32))
    plain = RL.Relighter(low_v, low_f, mats, env, normals='angle')
    mapped = RL.Relighter(low_v, low_f, mats, env, normals='angle', tracer=plain.tracer,
                          normal_map={'normal': bk['normal'], 'vt': bk['vt'], 'ft': bk['ft'], 'space': 'tangent'})
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(8, 0.0, 30.0, 3.0))[3]
    K = RL.default_K(800, 800)
    ro, rd = plain.camera_rays(pose, K, 800, 800)
    spread = 1.0 / float(K[0, 0])
    view = {'pixels': 800 * 800, 'hit_pixels': int(plain.surface(ro, rd)['idx'].numel()),
            'surface_with_map': timed(lambda: mapped.surface(ro, rd, spread=spread), a.reps),
            'surface_without_map': timed(lambda: plain.surface(ro, rd, spread=spread), a.reps)}
    view['with_over_without'] = round(view['surface_with_map']['ms'] / view['surface_without_map']['ms'], 3)
    out['surface_800x800'] = view
    line = json.dumps(out)
    print(line)
    if not a.no_write:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'bench_transfer.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
