#!/usr/bin/env python
"""Extract the Stage-I mesh of a checkpoint as a PLY (the reference's extract_mesh.py), optionally without its debris, or clean an existing PLY:
the connected components of the marching-cubes surface, selected by face count, on the device (nero_amd.mesh, nero_amd/csrc/mesh_clean.hip);
and optionally simplified by vertex clustering (nero_amd/csrc/mesh_simplify.hip), in both modes, after the clean-up.

    python scripts/extract_mesh.py --cfg configs/shape/syn/bell.yaml --model data/model/bell_shape/model.pth --resolution 512 \\
        --keep-largest --out data/meshes/bell.ply
    python scripts/extract_mesh.py --in data/meshes/bell.ply --min-face-ratio 0.01 --out data/meshes/bell_clean.ply
    python scripts/extract_mesh.py --in data/meshes/bell_clean.ply --target-faces 100000 --out data/meshes/bell_100k.ply

Extract mode (--cfg, --model): the steps of NeROShapeRenderer.extract_geometry on the box [-1, 1]^3 (SDF grid, marching cubes, the clean-up
when a rule is given), all on the device; only the final mesh is copied to the host.  Without --model the mesh is that of the freshly
initialised network (a dry run).
Clean-only mode (--in): reads the PLY, cleans it, writes --out.
Rules (they intersect; with none of them extract mode writes the mesh as marching cubes gave it and clean-only mode drops unreferenced
vertices only): --keep-largest [K] keeps the K (default 1) components with the most faces, ties towards the component that holds the smaller
vertex index; --min-faces N drops components with fewer faces; --min-face-ratio R drops those below that fraction of the largest component's
face count.
Simplification: --simplify-cell C clusters the vertices on a grid of cells of size C, in the units of the mesh the device holds (grid
indices in extract mode, the PLY's units in clean-only mode); --target-faces N chooses the smallest cell of the ladder
nero_amd.mesh.simplify_cells that leaves at most N faces.  One or the other.  The JSON line then holds `simplify`: the vertex and face
counts before and after, the chosen cell, its step k, and the number of duplicate faces removed.
Normals: --normals {angle,area} writes smooth per-vertex normals of the final mesh into the PLY (nero_amd.mesh.vertex_normals), turned
outwards whatever the winding; in both modes, after the clean-up and the simplification.
Prints one JSON line: the per-component table (vertices, faces, area, bounding box) before and after; --table-limit caps the rows listed
per table (largest first), the counts are always complete."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_cfg(path):
    text = open(path).read()
    if path.endswith('.json'):
        return json.loads(text)
    import yaml
    return yaml.safe_load(text)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--cfg')
    ap.add_argument('--model', '--ckpt', dest='model')
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--in', dest='inp', help='clean-only mode: the PLY to clean')
    ap.add_argument('--out', required=True)
    ap.add_argument('--keep-largest', type=int, nargs='?', const=1, default=None, metavar='K')
    ap.add_argument('--min-faces', type=int, default=0, metavar='N')
    ap.add_argument('--min-face-ratio', type=float, default=0.0, metavar='R')
    ap.add_argument('--simplify-cell', type=float, default=None, metavar='C')
    ap.add_argument('--target-faces', type=int, default=None, metavar='N')
    ap.add_argument('--normals', choices=['angle', 'area'], default=None,
                    help='write smooth vertex normals (nx, ny, nz) into the PLY, pointing outwards: face normals weighted by angle or by area')
    ap.add_argument('--table-limit', type=int, default=32)
    args = ap.parse_args(argv)
    if args.inp and (args.cfg or args.model):
        ap.error('--in cleans an existing PLY; --cfg / --model extract one: give one or the other')
    if not args.inp and not args.cfg:
        ap.error('give --cfg (and --model) to extract a mesh, or --in to clean an existing PLY')
    if args.simplify_cell is not None and args.target_faces is not None:
        ap.error('--simplify-cell and --target-faces both choose the cell: give one or the other')
    return args


def simplify_of(args):
    """the simplify_mesh_device arguments the command line asks for, None when it asks for none"""
    if args.simplify_cell is not None:
        return {'cell': args.simplify_cell}
    if args.target_faces is not None:
        return {'target_faces': args.target_faces}
    return None


def rules_of(args):
    """the clean_mesh_device rules the command line asks for, None when it asks for none"""
    rules = {}
    if args.keep_largest is not None:
        rules['keep'] = args.keep_largest
    if args.min_faces:
        rules['min_faces'] = args.min_faces
    if args.min_face_ratio:
        rules['min_face_ratio'] = args.min_face_ratio
    return rules or None


def report(cc, limit):
    rows = sorted(cc.table(), key=lambda r: (-r['n_faces'], r['component']))
    return {'components': cc.K, 'n_verts': int(cc.n_verts.sum()), 'n_faces': int(cc.n_faces.sum()), 'area': float(cc.area.sum()),
            'listed': min(limit, len(rows)), 'table': rows[:limit]}


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from nero_amd import mesh as M
    rules = rules_of(args)
    if args.inp:
        v, f = M.read_ply(args.inp)
        vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
        fd = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).cuda()
        to_world = lambda x: x.cpu().numpy()
    else:
        from nero_amd.renderer import NeROShapeRenderer
        cfg = load_cfg(args.cfg)
        net = NeROShapeRenderer({k: v for k, v in cfg.items() if k in NeROShapeRenderer.default_cfg}, training=False)
        if args.model:
            sd = torch.load(args.model, map_location='cpu')
            net.load_state_dict(sd.get('network_state_dict', sd))
        else:
            print('no --model: extracting the mesh of the freshly initialised network', file=sys.stderr)
        net = net.cuda().eval()
        lo, hi = (-1., -1., -1.), (1., 1., 1.)
        vd, fd = M.marching_cubes_device(net._sdf_grid(lo, hi, args.resolution, 2 ** 21, 1.0), 0.0)
        to_world = lambda x: M.index_to_world(x.cpu().numpy(), args.resolution, lo, hi)         # what extract_geometry returns
    out = {'out': args.out, 'mode': 'clean' if args.inp else 'extract', 'rules': rules}
    if rules is None and not args.inp:
        v2, f2 = vd, fd
        out['before'] = out['after'] = report(M.connected_components_device(vd, fd), args.table_limit)
    else:
        v2, f2, info = M.clean_mesh_device(vd, fd, **(rules or {}))
        out['before'] = report(info.components, args.table_limit)
        out['kept_components'] = [int(c) for c in torch.nonzero(info.keep)[:, 0].tolist()][:args.table_limit]
        out['after'] = report(M.connected_components_device(v2, f2), args.table_limit)
    simplify = simplify_of(args)
    if simplify is not None:
        n_before = {'n_verts': int(v2.shape[0]), 'n_faces': int(f2.shape[0])}
        v2, f2, sinfo = M.simplify_mesh_device(v2, f2, **simplify)
        out['simplify'] = {**simplify, 'before': n_before, 'after': {'n_verts': int(v2.shape[0]), 'n_faces': int(f2.shape[0])},
                           'cell': sinfo.cell, 'k': sinfo.k, 'n_survivors': sinfo.n_survivors, 'n_duplicates': sinfo.n_duplicates}
    if not args.inp:
        out['resolution'] = args.resolution
        out['table_space'] = 'grid index'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    vw = to_world(v2)
    normals = None
    if args.normals:                                                      # of the vertices the file holds, as float32, turned outwards
        normals, ninfo = M.vertex_normals(np.ascontiguousarray(vw, dtype=np.float32), f2, weight=args.normals, orient='outward', return_info=True)
        out['normals'] = dict(zip(('weight', 'refused_faces', 'faces_without_area', 'zero_normals'), [args.normals] + ninfo[:3].tolist()))
    M.write_ply(args.out, vw, f2, normals=normals)
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
