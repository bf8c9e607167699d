#!/usr/bin/env python
"""Texture baking on one MI355X (nero_amd/texture.py): three stages timed with device events, a warm-up, the median of --reps runs.

    raster + interpolate   nero_uv_raster + nero_uv_interp (including their count readbacks)
    regions + fill         nero_tex_regions + nero_tex_fill on the mask of that raster, 5 channels, pad 32
    bake                   the whole bake_materials (raster, interpolation, the material MLPs, quantisation, gutter, downsample)
at 1024 x ssaa 2 and 2048 x ssaa 2, on the 1280-triangle icosphere (built-in atlas) and on a ~200 k-triangle marching-cubes sphere (built-in
atlas laid out at the raster size: it does not fit at 1024).  Where scipy and sklearn are importable, the reference's own CPU formulation of
regions + fill (binary_dilation / binary_erosion / kd-tree, extract_materials_texture_map.py:136-149) is timed once on the same mask.
Writes profiles/bench_texture.json and prints it as one JSON line.

Bytes, from the shapes (N texels, n covered, F fill texels, C = 5): raster + interpolate writes the ids once and reads them twice (12 N), the
scan's flags and ranks (16 N) and 16 n of output; regions + fill moves 1 byte per texel four times (mask, row distances twice, regions), the
window staging re-reads the regions (16 + 2 pad)^2 / 256 times per texel, and the fill scans at most (2 pad + 1)^2 LDS bytes per fill texel."""
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


def timed(fn, reps, warmup=3):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for it in range(reps + warmup):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4), 'reps': reps}, out


def mc_sphere(res=160, radius=0.93):
    from nero_amd.mesh import marching_cubes_device
    g = torch.linspace(-1, 1, res, device='cuda')
    u = torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) - radius
    v, f = marching_cubes_device(u.contiguous(), 0.0)
    return (v / (res - 1) - 0.5).cpu().numpy(), f.cpu().numpy()          # radius ~0.46 around the origin


def cpu_reference(mask, tex, pad):
    try:
        from scipy.ndimage import binary_dilation, binary_erosion
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        return None
    t0 = time.perf_counter()
    inpaint = binary_dilation(mask, iterations=pad)
    inpaint[mask] = 0
    search = mask.copy()
    search[binary_erosion(search, iterations=3)] = 0
    sc, ic = np.stack(np.nonzero(search), -1), np.stack(np.nonzero(inpaint), -1)
    _, ind = NearestNeighbors(n_neighbors=1, algorithm='kd_tree').fit(sc).kneighbors(ic)
    tex[tuple(ic.T)] = tex[tuple(sc[ind[:, 0]].T)]
    return round((time.perf_counter() - t0) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-cpu-reference', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_texture.json'))
    args = ap.parse_args()
    from nero_amd import texture as TX
    from nero_amd.renderer import NeROMaterialRenderer
    from nero_amd.synthetic import icosphere, perturb_state
    assert torch.cuda.is_available(), 'bench_texture.py needs a GPU'
    ico = icosphere(3, 0.5, 0.15)
    meshes = {'icosphere_1280': (ico[0], np.ascontiguousarray(ico[1][:, ::-1])), 'mc_sphere': mc_sphere()}
    out = {'metric': 'texture_bake', 'device': torch.cuda.get_device_name(0), 'pad': 32, 'ssaa': 2, 'reps': args.reps}
    for mname, (v, f) in meshes.items():
        torch.manual_seed(6033)
        net = NeROMaterialRenderer({'database_name': 'syn/bell'}, is_train=False, mesh=(v, f))
        perturb_state(net, None)
        net = net.cuda()
        for size in args.sizes:
            H = size * 2
            try:
                vt, ft = TX.simple_atlas(v, f, size)
                laid = size
            except ValueError:
                vt, ft = TX.simple_atlas(v, f, H)
                laid = H
            vt_d, ft_d = torch.from_numpy(vt).cuda(), torch.from_numpy(ft).cuda()
            v_d, f_d = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).cuda()
            rec = {'triangles': int(len(f)), 'raster': f'{H}x{H}', 'atlas_laid_out_at': laid}
            rec['raster_interp'], (texel, pts, mask) = timed(
                lambda: TX.interpolate(TX.rasterize_uv(vt_d, ft_d, H, H), vt_d, ft_d, v_d, f_d, return_mask=True), args.reps)
            n = int(texel.shape[0])
            rec['covered_texels'] = n
            rec['raster_interp']['bytes'] = 28 * H * H + 16 * n
            tex0 = torch.randint(1, 256, (H, H, 5), dtype=torch.uint8, device='cuda')
            tex = tex0.clone()

            def gutter():
                tex.copy_(tex0)                                     # (the copy is inside the timed window: 2 x 5 bytes per texel)
                region = TX.gutter_regions(mask, 32, 3)
                TX.fill_gutter(tex, region, 32)
                return region
            rec['regions_fill'], region = timed(gutter, args.reps)
            rec['fill_texels'] = int((region == 3).sum())
            rec['search_texels'] = int((region == 2).sum())
            rec['bake'], _ = timed(lambda: net.extract_texture_maps(vt=vt_d, ft=ft_d, size=size, ssaa=2), args.reps)
            if not args.no_cpu_reference:
                rec['cpu_scipy_sklearn_regions_fill_ms'] = cpu_reference(mask.cpu().numpy() > 0, tex0.cpu().numpy(), 32)
            out[f'{mname}@{size}x2'] = rec
            del tex, tex0, region, texel, pts, mask
            torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
