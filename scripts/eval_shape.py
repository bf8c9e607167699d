"""Chamfer distance of an extracted mesh on the GPU (nero_amd/eval_shape.py), the reference's two procedures:

    python scripts/eval_shape.py --pr A.ply --gt B.ply
        eval_real_shape.py: nearest distances between the vertices (or points) of two PLY files.
    python scripts/eval_shape.py --pr A.ply --gt B.ply --samples 500000 [--seed S] [--iid]
        eval.md's full recipe for two MESHES: N points sampled on each surface on the GPU (nero_amd/surface.py, what eval.md gives to
        CloudCompare), then the same distances.  A PLY without faces is used as it is.
    python scripts/eval_shape.py --pr A.ply --gt B.ply --samples 500000 --exact
        the same two sample sets, each measured to the other MESH'S SURFACE (exact point-to-triangle distances through the tracer's BVH,
        CloudCompare's cloud-to-mesh distance) instead of to the other set's nearest sample: no floor from the sample spacing.  Both files
        must have faces.
    python scripts/eval_shape.py --mesh M.ply --views views.npz (--gt-points P.ply | --gt-depths D.npz)
        eval_synthetic_shape.py: the mesh's depth map in every view of views.npz (poses [n,3,4] world -> camera, Ks [n,3,3], hw [n,2]),
        back-projected and voxel-down-sampled, against the ground-truth points (the data set's eval_pts.ply) or the points made the same way
        from ground-truth depth maps (D.npz: depths [n,h,w], masks [n,h,w]).

Prints `<stem> <chamfer:.5f>` as the reference does.  Loading a data set's images and poses is not part of this project."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pr', type=str, help='predicted mesh or point cloud (PLY)')
    ap.add_argument('--gt', type=str, help='ground-truth mesh or point cloud (PLY)')
    ap.add_argument('--samples', type=int, default=None, metavar='N',
                    help='--pr/--gt: sample N points on the surface of every PLY that has faces (eval.md: 500000) instead of taking its '
                         'vertices; a PLY without faces is used as it is')
    ap.add_argument('--seed', type=int, default=0, help='--samples: seed of the sampler')
    ap.add_argument('--iid', action='store_true', help='--samples: independent draws instead of stratified ones')
    ap.add_argument('--exact', action='store_true',
                    help='--samples: measure every sample to the other mesh\'s surface (point to triangle) instead of to its nearest sample')
    ap.add_argument('--mesh', type=str, help='extracted mesh (PLY) for the synthetic procedure')
    ap.add_argument('--views', type=str, help='npz with poses [n,3,4], Ks [n,3,3], hw [n,2]')
    ap.add_argument('--gt-points', type=str, help='ground-truth eval points (PLY)')
    ap.add_argument('--gt-depths', type=str, help='npz with depths [n,h,w] and masks [n,h,w]')
    ap.add_argument('--voxel-size', type=float, default=0.01)
    ap.add_argument('--unproject-offset', type=float, default=0.0,
                    help='0 = the reference (integer pixel coordinates), 0.5 = through the pixel centres')
    ap.add_argument('--bvh-build', choices=('host', 'device'), default='host',
                    help='--mesh/--views and --exact: where the ray tracer builds its tree (device: on the GPU, same tree)')
    ap.add_argument('--batch_size', type=int, default=None, help='accepted for compatibility with the reference; nothing is batched')
    a = ap.parse_args(argv)
    real, syn = a.pr is not None or a.gt is not None, a.mesh is not None or a.views is not None
    if real == syn:
        ap.error('choose one procedure: --pr A.ply --gt B.ply, or --mesh M.ply --views views.npz with a ground truth')
    if real and (a.pr is None or a.gt is None):
        ap.error('the real-shape procedure needs both --pr and --gt')
    if a.samples is not None and (syn or a.samples < 1):
        ap.error('--samples N (N >= 1) belongs to the real-shape procedure, --pr A.ply --gt B.ply')
    if a.exact and a.samples is None:
        ap.error('--exact belongs to --pr A.ply --gt B.ply --samples N')
    if syn:
        if a.mesh is None or a.views is None:
            ap.error('the synthetic procedure needs both --mesh and --views')
        if (a.gt_points is None) == (a.gt_depths is None):
            ap.error('the synthetic procedure needs one ground truth: --gt-points P.ply or --gt-depths D.npz')
    return a


def has_faces(path):
    """whether the PLY file's header declares a non-empty face element"""
    from nero_amd import mesh as M
    with open(path, 'rb') as fh:
        return any(el['name'] == 'face' and el['count'] > 0 for el in M._read_header(fh)[1])


def _cloud(path, a):
    """the point set of one side of --pr/--gt: the file's vertices (or points), or with --samples N points sampled on its surface when it
    has faces (eval.md: 'sample points on the surface', on both meshes alike)"""
    from nero_amd import eval_shape as E
    if a.samples is None or not has_faces(path):
        return E.read_ply_points(path)
    from nero_amd import mesh as M
    from nero_amd.surface import sample_surface
    v, f = M.read_ply(path)
    return sample_surface(v, f, a.samples, seed=a.seed, stratified=not a.iid)


def main(argv=None):
    a = parse(argv)
    for path in (a.pr, a.gt, a.mesh, a.views, a.gt_points, a.gt_depths):
        if path is not None and not os.path.exists(path):
            sys.exit(f'eval_shape: {path} does not exist')
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    if a.pr is not None:
        stem = Path(a.pr).stem
        if a.exact:
            for path in (a.pr, a.gt):
                if not has_faces(path):
                    sys.exit(f'eval_shape: --exact measures to a surface, and {path} has no faces')
            chamfer = E.eval_meshes(M.read_ply(a.pr), M.read_ply(a.gt), n=a.samples, seed=a.seed, stratified=not a.iid, exact=True,
                                    bvh_build=a.bvh_build)
        else:
            chamfer = E.eval_point_clouds(_cloud(a.pr, a), _cloud(a.gt, a))
    else:
        stem = Path(a.mesh).stem
        v, f = M.read_ply(a.mesh)
        views = np.load(a.views)
        kw = dict(voxel_size=a.voxel_size, unproject_offset=a.unproject_offset, bvh_build=a.bvh_build)
        if a.gt_points is not None:
            kw['gt_points'] = E.read_ply_points(a.gt_points)
        else:
            gt = np.load(a.gt_depths)
            kw['gt_depths'], kw['gt_masks'] = gt['depths'], gt['masks']
        chamfer = E.eval_mesh(v, f, views['poses'], views['Ks'], views['hw'], **kw)
    print(f'{stem} {chamfer:.5f}')
    return chamfer


if __name__ == '__main__':
    main()
