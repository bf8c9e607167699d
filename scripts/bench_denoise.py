"""The denoiser on one MI355X (include/nero_hip_denoise.h, nero_amd/denoise.py), at 800 x 800 and 1600 x 1600 on the
bench mesh of bench_relight.py (a bumpy icosphere of 81 920 triangles, random per-vertex materials, a 256 x 512 random map with a hot
texel).  Everything that is compared is alternated in one process on the same inputs (HIP events, median over --reps after a warm-up,
with minimum and maximum):
  * the variance pass and each a-trous step (1, 2, 4, 8, 16) on the specular signal's records (G = 4), with the rate of the BYTE MODEL:
    25 taps (49 for the variance window) x 48 bytes (a 32-byte guide record and a 16-byte signal record; 64 with G = 4) per pixel per
    pass.  That is what the taps ask of the memory system, not what reaches HBM: neighbouring pixels ask for the same records;
  * the whole filter of a view's three signals (Relighter._denoise: packing in torch, 3 x (variance + 5 passes)), and the 18 kernel calls
    alone;
  * one a-trous step in plain torch (sums over shifted slices of the padded planes) on the same records, with its distance from the kernel;
  * whole views (Relighter.render, wall time, minimum of two runs after a warm-up run) and their RMSE over the covered pixels to a
    1024 + 1024 render: 128 + 128 undenoised against 16 + 16 and 32 + 32 denoised, and those two undenoised, with and without one bounce.
Prints one JSON line and writes it to profiles/bench_denoise.json.

    python scripts/bench_denoise.py [--reps 7] [--sizes 800 1600] [--no-write]"""
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

STEPS = (1, 2, 4, 8, 16)
C5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
C3 = (0.25, 0.5, 0.25)


def alternate(fns, reps, warmup=2):
    """the callables of `fns` in turn, reps + warmup rounds -> (median, min, max) ms of each (HIP events)"""
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
    return [(round(statistics.median(m), 4), round(min(m), 4), round(max(m), 4)) for m in ms]


def _shift(x, oy, ox, pad):
    """x [h + 2 pad, w + 2 pad, C] -> the [h, w, C] window moved by (oy, ox)"""
    h, w = x.shape[0] - 2 * pad, x.shape[1] - 2 * pad
    return x[pad + oy:pad + oy + h, pad + ox:pad + ox + w]


def torch_atrous(guide, sig, h, w, step, k, sigma_l, sigma_p, sigma_g):
    """nero_denoise_atrous in plain torch: the planes padded with invalid pixels, one shifted slice per tap -> signal [h w,4]"""
    G = guide.shape[1] - 8
    pad = 2 * step
    P = lambda x: torch.nn.functional.pad(x.reshape(h, w, -1).permute(2, 0, 1), (pad, pad, pad, pad)).permute(1, 2, 0)
    g, s = P(guide), P(sig)
    g0, s0 = guide.reshape(h, w, -1), sig.reshape(h, w, 4)
    lum = lambda x: (0.2126 * x[..., 0] + 0.7152 * x[..., 1]) + 0.0722 * x[..., 2]
    va, vb = torch.zeros(h, w, device=sig.device), torch.zeros(h, w, device=sig.device)
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            c = C3[oy + 1] * C3[ox + 1]
            ok = _shift(g, oy, ox, pad)[..., 3] != 0
            va = va + torch.where(ok, c * _shift(s, oy, ox, pad)[..., 3], torch.zeros_like(va))
            vb = vb + ok.float() * c
    valid = g0[..., 3] != 0
    den = sigma_l * torch.sqrt(va / torch.where(valid, vb, torch.ones_like(vb))) + 1e-6
    lum_p = lum(s0)
    acc = torch.zeros(h, w, 5, device=sig.device)
    for ty in range(5):
        for tx in range(5):
            gq, sq = _shift(g, (ty - 2) * step, (tx - 2) * step, pad), _shift(s, (ty - 2) * step, (tx - 2) * step, pad)
            wn = torch.clamp((g0[..., 0:3] * gq[..., 0:3]).sum(-1), min=0.0)
            for _ in range(k):
                wn = wn * wn
            wt = wn * torch.exp(-(g0[..., 0:3] * (gq[..., 4:7] - g0[..., 4:7])).sum(-1).abs() / sigma_p)
            if G == 4:
                wt = wt * torch.exp(-((g0[..., 8:12] - gq[..., 8:12]) ** 2).sum(-1) / (sigma_g * sigma_g))
            wt = (C5[ty] * C5[tx]) * wt * torch.exp(-(lum_p - lum(sq)).abs() / den)
            wt = torch.where(valid & (gq[..., 3] != 0), wt, torch.zeros_like(wt))
            acc[..., 0] += wt
            acc[..., 1:4] += wt[..., None] * sq[..., 0:3]
            acc[..., 4] += wt * wt * sq[..., 3]
    ok = valid & (acc[..., 0] > 0)
    sw = torch.where(ok, acc[..., 0], torch.ones_like(va))
    out = torch.cat([acc[..., 1:4] / sw[..., None], (acc[..., 4] / (sw * sw))[..., None]], -1)
    return torch.where(ok[..., None], out, s0).reshape(h * w, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[800, 1600])
    ap.add_argument('--no-write', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import denoise as DN
    from nero_amd import relight as RL
    from nero_amd.synthetic import icosphere
    v, f = icosphere(6, 0.5, 0.15)
    g = np.random.default_rng(0)
    mats = {'metallic': g.uniform(0, 1, (len(v), 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (len(v), 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (len(v), 3)).astype(np.float32)}
    env = torch.from_numpy(g.uniform(0.2, 1.2, (256, 512, 3)).astype(np.float32))
    env[60, 300] *= 1000.0
    rl = RL.Relighter(v, f, mats, env, convention='blender')
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(8, 0.0, 30.0, 3.0))[3]
    out = {'mesh_triangles': int(len(f)), 'reps': a.reps, 'device': torch.cuda.get_device_name(0),
           'byte_model': '25 taps x 48 bytes per pixel per a-trous pass (64 with G = 4), 49 taps for the variance window: what the taps ask for, not HBM traffic'}
    for n in a.sizes:
        K = RL.default_K(n, n)
        res = {}
        # ---- the records of one 16 + 16 view with one bounce -------------------------------------------------------------------------
        ro, rd = rl.camera_rays(pose, K, n, n)
        sf = rl.surface(ro, rd)
        idx = sf['idx']
        rand_d, rand_s = RL.pixel_rotations(idx, 0)
        pt = RL.point_records(sf['pts'], -rd[idx], sf['normal'], RL.estimator_materials(sf['mat5']), rand_d, rand_s)
        got = RL.relight_points(rl.tracer, pt, rl._table(16), rl._table(16), rl.env, rl.convention, rl.rot, None, rl.geometry_type, None, bounces=1,
                                mesh=(rl.verts, rl.tris.int(), rl.mat5, rl.normals), key=RL.pixel_keys(idx, 0))
        dn = DN.options(True, 0.015 * float((rl.verts.max(0).values - rl.verts.min(0).values).norm()))
        full = lambda x: torch.zeros(n * n, x.shape[1], device=rl.device).index_copy_(0, idx, x)
        m5 = sf['mat5']
        lum = (0.2126 * m5[:, 2:3] + 0.7152 * m5[:, 3:4]) + 0.0722 * m5[:, 4:5]
        guide = DN.pack_guides(full(sf['pts']), full(sf['normal']), sf['hit'].reshape(-1), full(torch.cat([m5[:, 1:2], m5[:, 0:1], lum, torch.zeros_like(lum)], -1)))
        sig = DN.estimate_variance(guide, DN.pack_signal(full(got[2])), n, n, dn['normal_pow2'], dn['sigma_p'], dn['sigma_g'])
        buf = torch.empty_like(sig)
        kw = dict(normal_pow2=dn['normal_pow2'], sigma_p=dn['sigma_p'], sigma_g=dn['sigma_g'])
        res['hit_pixels'], res['pixels'] = int(idx.numel()), n * n
        # ---- the passes ---------------------------------------------------------------------------------------------------------------
        fns = [lambda: DN.estimate_variance(guide, sig, n, n, out=buf, **kw)]
        fns += [lambda s=s: DN.atrous_pass(guide, sig, n, n, s, sigma_l=dn['sigma_l'], out=buf, **kw) for s in STEPS]
        fns += [lambda: DN.denoise_records(guide, sig, n, n, dn['iterations'], dn['sigma_l'], **kw),
                lambda: [DN.denoise_records(gd, sig, n, n, dn['iterations'], dn['sigma_l'], **kw) for gd in (guide, guide, guide)],
                lambda: rl._denoise(dn, n, n, sf, got, 1),
                lambda: torch_atrous(guide, sig, n, n, 1, dn['normal_pow2'], dn['sigma_l'], dn['sigma_p'], dn['sigma_g'])]
        names = ['variance'] + [f'atrous_step_{s}' for s in STEPS] + ['one_signal_6_kernels', 'three_signals_18_kernels', 'three_signals_with_packing',
                                                                      'torch_atrous_step_1']
        taps = [49] + [25] * len(STEPS)
        for k, (name, (med, lo, hi)) in enumerate(zip(names, alternate(fns, a.reps))):
            res[name] = {'ms': med, 'ms_min_max': [lo, hi]}
            if k < len(taps):
                model = res['hit_pixels'] * taps[k] * 64
                res[name].update(model_bytes=model, model_GB_per_s=round(model / med / 1e6, 1))
        ker, ref = DN.atrous_pass(guide, sig, n, n, 1, sigma_l=dn['sigma_l'], **kw), torch_atrous(guide, sig, n, n, 1, dn['normal_pow2'], dn['sigma_l'],
                                                                                               dn['sigma_p'], dn['sigma_g'])
        res['torch_atrous_step_1']['max_abs_distance_from_kernel'] = float((ker - ref).abs().max())
        res['torch_atrous_step_1']['over_kernel'] = round(res['torch_atrous_step_1']['ms'] / res['atrous_step_1']['ms'], 1)
        del guide, sig, buf, got, pt, ker, ref
        # ---- whole views --------------------------------------------------------------------------------------------------------------
        for b in (0, 1):
            conv = rl.render(pose, K, n, n, samples=(1024, 1024), bounces=b)
            hit = conv['alpha'][..., 0] > 0
            views = {}
            for s, d in ((128, None), (16, None), (16, True), (32, None), (32, True)):
                runs = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    img = rl.render(pose, K, n, n, samples=(s, s), bounces=b, denoise=d)
                    torch.cuda.synchronize()
                    runs.append(round((time.perf_counter() - t) * 1e3, 2))
                views[f'{s}+{s}' + (' denoised' if d else '')] = {
                    'ms_min_of_2_after_warmup': min(runs[1:]), 'ms_all_runs': runs,
                    'rmse_to_1024+1024': float(((img['rgb_lin'][hit] - conv['rgb_lin'][hit]).double() ** 2).mean().sqrt())}
            res[f'view_bounces_{b}'] = views
            del conv, img
        out[f'{n}x{n}'] = res
    line = json.dumps(out)
    print(line)
    if not a.no_write:
        os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'bench_denoise.json'), 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
