#!/usr/bin/env python
"""Bake the Stage-II materials into albedo / metallic / roughness texture maps and write the textured OBJ (the reference's
extract_materials_texture_map.py) through nero_amd.texture -- no xatlas / nvdiffrast / scipy / sklearn / cv2.

    python scripts/extract_texture_maps.py --cfg configs/material/syn/bell.yaml --ckpt data/model/bell_material/model.pth --out data/materials/bell
    python scripts/extract_texture_maps.py --mesh mesh.ply --ckpt model.pth --uv atlas.npz --size 2048 --out out_dir
    python scripts/extract_texture_maps.py --mesh mesh.ply --ckpt model.pth --atlas charts --size 2048 --out out_dir

--cfg: the material YAML (or JSON); its `mesh` entry names the Stage-I mesh unless --mesh does.  --ckpt: a trainer checkpoint (the
`network_state_dict` entry) or a bare state dict; without it the maps show the freshly initialised network (a dry run of the pipeline).
--uv: an .npz with `vt` [nvt, 2] in [0, 1] and `ft` [T, 3] from any unwrapper (xatlas: `vmapping, ft, vt = xatlas.parametrize(v, f)`); without it
--atlas chooses the built-in one: `triangles` (the default), one chart per triangle, which needs size >= 4 * ceil(sqrt(T / 2)) -- a fallback for
small or decimated meshes; `charts`, the projection atlas of nero_amd.texture.chart_atlas (--gutter texels between charts), for a mesh as it
comes from the clean-up.  With `charts` the number of charts, the scale (texels per world unit), the fill and the texels covered twice are
printed, a warning is given when any texel is covered twice, and the atlas is saved as <name>_atlas.npz next to the OBJ (vt, ft, vt_vertex,
vt_chart, chart, rects, scale).  --ao-samples N (a power of two in [8, 1024]; 0, the default: no AO map) also bakes an ambient-occlusion map
from N shadow rays per texel, no longer than --ao-radius (default: unbounded) and started --ao-bias above the surface; it is written as
feat3_<cas>.png and named by a map_Ka line of the MTL.

    python scripts/extract_texture_maps.py --mesh dense.ply --ckpt model.pth --target-faces 100000 --atlas charts --normal-map --out out_dir

--target-faces N (simplify the mesh to at most N faces first) or --low-mesh L.ply (a simplified mesh made elsewhere) bake the asset of the
SIMPLIFIED mesh with nero_amd.transfer.bake_asset: every texel is projected onto the dense mesh, the networks are evaluated there, and the
OBJ holds the simplified mesh.  --normal-map also writes the dense mesh's shading normals as feat4_<cas>.png (`norm` in the MTL, with the
space and the frame mode in a comment): --normal-space tangent (the default) or object, --max-dist D bounds how far a texel may reach for
the dense surface.  Without --uv the atlas is --atlas as above (--gutter applies to `charts`; `triangles`, the default, holds
2 (size // 4)^2 faces and raises naming the smallest workable --size otherwise: 100 000 faces want --atlas charts).  --normal-map alone bakes on the mesh itself (a flat map).  A --uv atlas must then belong to the simplified mesh; no AO
map is baked on this path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_cfg(path):
    text = open(path).read()
    if path.endswith('.json'):
        return json.loads(text)
    import yaml
    return yaml.safe_load(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--cfg')
    ap.add_argument('--ckpt')
    ap.add_argument('--mesh', help='PLY of the Stage-I mesh (overrides the cfg entry)')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--ssaa', type=int, default=2, choices=(1, 2))
    ap.add_argument('--pad', type=int, default=32)
    ap.add_argument('--uv', help='.npz holding vt and ft')
    ap.add_argument('--atlas', choices=('triangles', 'charts'), default='triangles', help='the built-in atlas used without --uv')
    ap.add_argument('--gutter', type=int, default=4, help='texels between the charts of --atlas charts')
    ap.add_argument('--ao-samples', type=int, default=0, help='shadow rays per texel of the ambient-occlusion map; 0: no AO map')
    ap.add_argument('--ao-radius', type=float, default=None, help='longest shadow ray (default: unbounded)')
    ap.add_argument('--ao-bias', type=float, default=1e-4, help='shadow rays start this far above the surface')
    ap.add_argument('--target-faces', type=int, default=None, help='simplify the mesh to at most this many faces and bake the asset of that mesh')
    ap.add_argument('--low-mesh', help='PLY of a simplified mesh to bake the asset of')
    ap.add_argument('--normal-map', action='store_true', help="also bake the dense mesh's normals into a normal map")
    ap.add_argument('--normal-space', choices=('tangent', 'object'), default='tangent')
    ap.add_argument('--max-dist', type=float, default=None, help='how far a texel may reach for the dense surface (default: no limit)')
    ap.add_argument('--out', required=True)
    ap.add_argument('--name', default='mesh_0')
    args = ap.parse_args(argv)
    if not (args.cfg or args.mesh):
        ap.error('give --cfg (with a mesh entry) or --mesh')
    from nero_amd import texture as TX
    from nero_amd.mesh import read_ply
    from nero_amd.renderer import NeROMaterialRenderer
    cfg = load_cfg(args.cfg) if args.cfg else {}
    mesh_path = args.mesh or cfg['mesh']
    v, f = read_ply(mesh_path)
    net = NeROMaterialRenderer({k: cfg[k] for k in ('shader_cfg', 'database_name') if k in cfg}, is_train=False, mesh=(v, f))
    if args.ckpt:
        sd = torch.load(args.ckpt, map_location='cpu')
        net.load_state_dict(sd.get('network_state_dict', sd))
    else:
        print('no --ckpt: baking the freshly initialised network', file=sys.stderr)
    net = net.cuda().eval()
    vt = ft = None
    if args.uv:
        z = np.load(args.uv)
        vt, ft = z['vt'], z['ft']
    if args.target_faces is not None and args.low_mesh:
        ap.error('give --target-faces or --low-mesh, not both')
    if args.target_faces is not None or args.low_mesh or args.normal_map:
        if args.ao_samples > 0:
            ap.error('no ambient-occlusion map is baked on the transferred asset: drop --ao-samples')
        from nero_amd import transfer
        lv, lf = read_ply(args.low_mesh) if args.low_mesh else (None, None)
        maps = transfer.bake_asset(net, verts=lv, tris=lf, target_faces=args.target_faces, vt=vt, ft=ft, size=args.size, ssaa=args.ssaa, pad=args.pad,
                                   atlas=args.atlas, gutter=args.gutter, space=args.normal_space, max_dist=args.max_dist)
        if not args.normal_map:
            maps.pop('normal')
        obj = TX.write_textured_obj(args.out, maps['verts'], maps['tris'], maps['vt'], maps['ft'], maps, name=args.name)
        print(json.dumps({'obj': obj, 'size': args.size, 'ssaa': args.ssaa, 'pad': args.pad, 'source_triangles': int(len(f)),
                          'triangles': int(maps['tris'].shape[0]), 'covered_texels': int(maps['mask'].sum()),
                          'atlas': 'given' if args.uv else ('chart_atlas' if args.atlas == 'charts' else 'simple_atlas'),
                          'normal_map': bool(args.normal_map), 'normal_space': args.normal_space, 'normals': maps['normals'],
                          'unmatched': maps['unmatched'], 'max_moved': maps['max_moved'], 'max_dist': args.max_dist}))
        return
    info = None
    if vt is None and args.atlas == 'charts':
        vt, ft, info = TX.chart_atlas(net.mesh_vertices, net.mesh_triangles, args.size, gutter=args.gutter)
    ao = {'samples': args.ao_samples, 'radius': args.ao_radius, 'bias': args.ao_bias} if args.ao_samples > 0 else None
    maps = net.extract_texture_maps(vt=vt, ft=ft, size=args.size, ssaa=args.ssaa, pad=args.pad, ao=ao)
    obj = TX.write_textured_obj(args.out, net.mesh_vertices, net.mesh_triangles, maps['vt'], maps['ft'], maps, name=args.name)
    report = {'obj': obj, 'size': args.size, 'ssaa': args.ssaa, 'pad': args.pad, 'triangles': int(len(f)),
              'covered_texels': int(maps['mask'].sum()), 'atlas': 'given' if args.uv else ('chart_atlas' if info else 'simple_atlas')}
    if ao is not None:
        report.update(ao_samples=args.ao_samples, ao_radius=args.ao_radius, ao_bias=args.ao_bias)
    if info is not None:
        npz = os.path.join(args.out, args.name + '_atlas.npz')
        host = lambda x: x.cpu().numpy()
        np.savez(npz, vt=host(vt), ft=host(ft), vt_vertex=host(info.vt_vertex), vt_chart=host(info.vt_chart), chart=host(info.chart),
                 rects=info.rects, scale=np.float64(info.scale))
        report.update(charts=info.n_charts, scale=info.scale, fill=round(info.fill, 4), overlap_texels=info.overlap_texels,
                      chartless_faces=info.charts.n_chartless, gutter=args.gutter, atlas_npz=npz)
        print(f'chart atlas: {info.n_charts} charts, {info.scale:.6g} texels per unit, fill {info.fill:.3f}, {info.overlap_texels} texels '
              f'covered twice', file=sys.stderr)
        if info.overlap_texels > 0:
            print(f'warning: {info.overlap_texels} texel centres are covered by more than one triangle: a chart folds over itself in its '
                  f'projection, and the lowest face wins there', file=sys.stderr)
    print(json.dumps(report))


if __name__ == '__main__':
    main()
