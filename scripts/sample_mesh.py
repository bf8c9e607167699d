"""Points sampled on the surface of a mesh on the GPU (nero_amd/surface.py), written as a PLY point cloud: what the reference's eval.md
does with CloudCompare ("sample points on the surface.  We sample 500k points on the mesh in default") ahead of eval_real_shape.py.

    python scripts/sample_mesh.py --mesh M.ply --n 500000 --out P.ply [--seed S] [--iid]

Every triangle is chosen in proportion to its area.  The same mesh, --n, --seed and mode give the same file on every run."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mesh', type=str, required=True, help='triangle mesh (PLY)')
    ap.add_argument('--n', type=int, default=500000, help='number of points')
    ap.add_argument('--out', type=str, required=True, help='point cloud to write (PLY, float x y z)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--iid', action='store_true', help='independent draws instead of stratified ones')
    a = ap.parse_args(argv)
    if a.n < 1:
        ap.error('--n must be at least 1')
    return a


def main(argv=None):
    a = parse(argv)
    if not os.path.exists(a.mesh):
        sys.exit(f'sample_mesh: {a.mesh} does not exist')
    from eval_shape import has_faces
    if not has_faces(a.mesh):
        sys.exit(f'sample_mesh: {a.mesh} has no faces: there is no surface to sample')
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    from nero_amd.surface import sample_surface
    v, f = M.read_ply(a.mesh)
    pts = sample_surface(v, f, a.n, seed=a.seed, stratified=not a.iid)
    E.write_ply_points(a.out, pts)
    print(f'{a.out}: {len(pts)} points on {len(f)} triangles')


if __name__ == '__main__':
    main()
