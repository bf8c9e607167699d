"""CPU tier: the restatement the GPU clean-up tests compare against (tests/mesh_clean_ref.py) pinned on the analytic fields of
tests/mcubes_ref.py, the selection rules on hand-made statistics (nero_amd.mesh.select_components against the restatement's), and the
command line of scripts/extract_mesh.py.  The script's clean-only mode itself runs the HIP kernels, so its PLY round trip cannot run here: it
is test_script_cleans_a_ply in tests/test_mesh_clean_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import mcubes_ref as R
from tests import mesh_clean_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name,faces', [('sphere', None), ('torus', None), ('two_spheres', [5420, 7396])])
def test_components_of_the_analytic_fixtures(name, faces):
    v, f = MR.mesh_of(name)
    s = MR.ref_stats(name)
    assert s['K'] == (len(faces) if faces else 1)
    assert int(s['n_verts'].sum()) == len(v) and int(s['n_faces'].sum()) == len(f)
    if faces:
        assert s['n_faces'].tolist() == faces and len(f) == 12816
    # canonical numbering: component c's smallest vertex increases with c, and vertex 0 is in component 0
    first = [int(np.nonzero(s['comp'] == c)[0][0]) for c in range(s['K'])]
    assert first == sorted(first) and first[0] == 0
    assert np.array_equal(MR.labels(s['comp']), np.asarray(first, np.int32)[s['comp']])


def test_statistics_of_two_spheres():
    v, f = MR.mesh_of('two_spheres')
    s = MR.ref_stats('two_spheres')
    # marching-cubes spheres of radius 12 and 14: the areas within 2 % of 4 pi r^2, the boxes within a voxel of centre +- r
    for c, (centre, r) in enumerate([((18.2, 19.6, 17.7), 12.0), ((50.3, 19.4, 17.9), 14.0)]):
        assert abs(s['area'][c] / (4 * np.pi * r * r) - 1) < 0.02
        assert np.abs(s['bbox_min'][c] - (np.asarray(centre) - r)).max() < 1.0
        assert np.abs(s['bbox_max'][c] - (np.asarray(centre) + r)).max() < 1.0
    assert s['area'].dtype == np.float64 and s['bbox_min'].dtype == np.float32


def test_keeping_the_largest_of_two_spheres_gives_a_closed_sphere():
    v, f = MR.mesh_of('two_spheres')
    v2, f2, vmap = MR.clean(v, f, keep='largest')
    assert len(f2) == 7396 and R.euler_characteristic(v2, f2) == 2
    assert (vmap >= 0).sum() == len(v2) and np.array_equal(v2, v[vmap >= 0])
    assert np.array_equal(np.diff(vmap[vmap >= 0]), np.ones(len(v2) - 1, np.int32))          # the survivors keep their order
    assert v2[:, 0].min() > 35.0                                                              # the sphere of radius 14 at x = 50.3
    w, g, _ = MR.clean(v, f)                                                                  # no rule: nothing to drop here
    assert np.array_equal(w, v) and np.array_equal(g, f)


def test_the_tube_is_one_long_thin_component():
    v, f = MR.mesh_of('tube')
    assert (len(v), len(f)) == (5208, 10412)
    assert MR.ref_stats('tube')['K'] == 1 and R.euler_characteristic(v, f) == 2
    assert MR.graph_eccentricity(len(v), f, 0) == 265


@pytest.mark.parametrize('shape', sorted(MR.RANDOM_SHAPES))
def test_random_fields_have_many_components(shape):
    assert MR.ref_stats(shape)['K'] >= MR.RANDOM_SHAPES[shape]


def test_compaction_drops_unreferenced_vertices_and_remaps():
    v = np.arange(21, dtype=np.float32).reshape(7, 3)
    f = np.array([[1, 2, 4], [4, 2, 1], [5, 6, 6]], np.int32)          # vertices 0 and 3 unreferenced; a duplicate and a degenerate face
    s = MR.stats(v, f)
    assert s['K'] == 4 and s['comp'].tolist() == [0, 1, 1, 2, 1, 3, 3]
    assert s['n_verts'].tolist() == [1, 3, 1, 2] and s['n_faces'].tolist() == [0, 2, 0, 1] and s['area'][3] == 0.0
    v2, f2, vmap = MR.compact(v, f, s['comp'], np.ones(4, bool))
    assert vmap.tolist() == [-1, 0, 1, -1, 2, 3, 4] and f2.tolist() == [[0, 1, 2], [2, 1, 0], [3, 4, 4]]
    v2, f2, vmap = MR.compact(v, f, s['comp'], np.array([1, 0, 1, 1], bool))
    assert vmap.tolist() == [-1, -1, -1, -1, -1, 0, 1] and f2.tolist() == [[0, 1, 1]] and np.array_equal(v2, v[5:])
    v2, f2, vmap = MR.compact(v, f, s['comp'], np.zeros(4, bool))
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and (vmap == -1).all()


RULES = [({}, [1, 1, 1, 1, 1, 1]), ({'keep': 'largest'}, [0, 1, 0, 0, 0, 0]), ({'keep': 1}, [0, 1, 0, 0, 0, 0]),
         ({'keep': 2}, [0, 1, 0, 1, 0, 0]),                            # 9 faces twice: the smaller number wins the tie
         ({'keep': 3}, [0, 1, 0, 1, 1, 0]), ({'keep': 0}, [0, 0, 0, 0, 0, 0]), ({'keep': 99}, [1, 1, 1, 1, 1, 1]),
         ({'min_faces': 5}, [0, 1, 0, 1, 1, 1]), ({'min_faces': 9}, [0, 1, 0, 1, 1, 0]), ({'min_face_ratio': 0.25}, [0, 1, 0, 1, 1, 1]),
         ({'min_face_ratio': 0.26}, [0, 1, 0, 1, 1, 0]), ({'min_face_ratio': 1.0}, [0, 1, 0, 0, 0, 0]),
         ({'keep': 3, 'min_faces': 10}, [0, 1, 0, 0, 0, 0]),           # intersection, not "the three largest of those above 10"
         ({'keep': 5, 'min_face_ratio': 0.2, 'min_faces': 6}, [0, 1, 0, 1, 1, 0])]


@pytest.mark.parametrize('rules,want', RULES)
def test_selection_rules_on_handmade_statistics(rules, want):
    from nero_amd.mesh import select_components
    n_faces = [4, 20, 0, 9, 9, 5]
    assert MR.select(n_faces, **rules).tolist() == [bool(x) for x in want]
    got = select_components(torch.tensor(n_faces, dtype=torch.int32), **rules)
    assert got.dtype == torch.bool and got.tolist() == [bool(x) for x in want]


def test_selection_rules_refuse_bad_arguments_and_accept_no_components():
    from nero_amd.mesh import select_components
    n = torch.tensor([3, 1], dtype=torch.int32)
    for bad in ({'keep': 'biggest'}, {'keep': -1}, {'keep': 1.5}, {'keep': True}, {'min_faces': -1}, {'min_face_ratio': 1.5}):
        with pytest.raises(ValueError):
            select_components(n, **bad)
    assert select_components(torch.zeros(0, dtype=torch.int32), keep='largest', min_face_ratio=0.5).shape == (0,)
    assert MR.select([], keep=2).shape == (0,)


def test_script_command_line():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import extract_mesh as E
    finally:
        sys.path.pop(0)
    a = E.parse_args(['--in', 'a.ply', '--out', 'b.ply', '--keep-largest'])
    assert E.rules_of(a) == {'keep': 1}
    a = E.parse_args(['--in', 'a.ply', '--out', 'b.ply', '--keep-largest', '3', '--min-faces', '40', '--min-face-ratio', '0.01'])
    assert E.rules_of(a) == {'keep': 3, 'min_faces': 40, 'min_face_ratio': 0.01}
    a = E.parse_args(['--cfg', 'c.yaml', '--model', 'm.pth', '--resolution', '128', '--out', 'b.ply'])
    assert E.rules_of(a) is None and a.resolution == 128
    for bad in (['--out', 'b.ply'], ['--in', 'a.ply', '--cfg', 'c.yaml', '--model', 'm.pth', '--out', 'b.ply'], ['--in', 'a.ply']):
        with pytest.raises(SystemExit):
            E.parse_args(bad)
