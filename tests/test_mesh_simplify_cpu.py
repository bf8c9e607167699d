"""CPU tier: the numpy restatement of the mesh simplification (tests/mesh_simplify_ref.py) pinned on the analytic fixtures and on the
values a prototype of the definition gave, its invariants on every fixture, the face-budget search against a linear scan, the C surface of
nero_mesh_simplify_* as far as it goes without a device (symbols, workspace sizes, refused arguments), the hand-off to simple_atlas, and the
command line.  The kernels themselves: tests/test_mesh_simplify_gpu.py."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

from tests import mcubes_ref as R
from tests import mesh_clean_ref as MR
from tests import mesh_simplify_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ['sphere', 'torus', 'two_spheres', 'tube', 'box'] + sorted(MR.RANDOM_SHAPES)


def mesh_of(name):
    return S.box_mesh() if name == 'box' else MR.mesh_of(name)


# ---- pinned values ----------------------------------------------------------------------------------------------------------------------
def test_sphere_and_torus_at_cell_2():
    o = S.simplify(*mesh_of('sphere'), 2.0)
    assert (len(o['verts']), len(o['tris']), o['n_duplicates']) == (1432, 2860, 0) and R.euler_characteristic(o['verts'], o['tris']) == 2
    o = S.simplify(*mesh_of('torus'), 2.0)
    assert (len(o['verts']), len(o['tris'])) == (2068, 4136) and R.euler_characteristic(o['verts'], o['tris']) == 0


def test_random_field_has_duplicates_of_both_kinds():
    v, f = mesh_of((24, 20, 18))
    o = S.simplify(v, f, 2.0, dedup=False)
    t = o['tris']
    assert o['n_survivors'] == len(t) == 4760 and o['n_duplicates'] == 0
    rot = np.stack([np.roll(x, -int(np.argmin(x))) for x in t])       # equal up to a rotation = the same face with the same winding
    assert len(np.unique(rot, axis=0)) == 4739 and len(np.unique(np.sort(t, axis=1), axis=0)) == 4195
    d = S.simplify(v, f, 2.0)
    assert d['n_duplicates'] == 565 >= 100 and len(d['tris']) == 4195  # the de-duplication tests cannot pass vacuously


def test_box_fixture_and_the_quality_of_the_quadric_placement():
    v, f = S.box_mesh()
    assert (len(v), len(f)) == (2066, 4128)
    want = {2: (0.0435, 0.0167), 3: (0.0737, 0.0145), 4: (0.3073, 0.0462)}
    for cell, (dm, dq) in want.items():
        mean = S.box_surface_distance(S.simplify(v, f, cell, placement='mean')['verts'])
        quad = S.box_surface_distance(S.simplify(v, f, cell, placement='quadric')['verts'])
        assert abs(mean - dm) < 5e-5 and abs(quad - dq) < 5e-5, (cell, mean, quad)
        assert quad / mean <= 0.5, (cell, quad / mean)


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', [1.0, 1.5, 2.0, 3.0])
@pytest.mark.parametrize('name', FIXTURES, ids=str)
def test_invariants_of_the_restatement(name, cell):
    v, f = mesh_of(name)
    for placement in ('quadric', 'mean'):
        o = S.simplify(v, f, cell, placement=placement)
        x, t, ijk = o['verts'], o['tris'].astype(np.int64), o['ijk']
        # every output vertex inside its cell's closed box
        lo, hi = o['origin'][None] + ijk * cell, o['origin'][None] + (ijk + 1) * cell
        assert (x >= lo).all() and (x <= hi).all()
        assert np.array_equal(o['cell_key'], (ijk[:, 0] << 42) | (ijk[:, 1] << 21) | ijk[:, 2]) and (np.diff(o['cell_key']) > 0).all()
        # vmap: every input vertex in its output vertex's cell; exactly the used cells are output
        _, key, ok = S.vertex_keys(v, cell, o['origin'])
        assert ok.all()
        ref_d = (o['vmap'] >= 0)
        assert np.array_equal(o['cell_key'][o['vmap'][ref_d]], key[ref_d])
        assert np.array_equal(np.unique(o['vmap'][ref_d]), np.arange(len(x)))
        assert not np.isin(key[~ref_d], o['cell_key']).any()
        # fmap: the kept faces, in their order, renumbered by vmap with the winding kept
        kept = np.nonzero(o['fmap'] >= 0)[0]
        assert np.array_equal(o['fmap'][kept], np.arange(len(t)))     # face order preserved
        assert np.array_equal(o['vmap'][f[kept]], t)
        assert len(np.unique(t.ravel())) == len(x)                    # every output vertex is used by an output face ...
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
        assert len(np.unique(np.sort(t, axis=1), axis=0)) == len(t)   # no two faces share a vertex set
        # the faces that went: collapsed (two corners in one cell) or a later copy of a kept vertex set
        gone = np.nonzero(o['fmap'] < 0)[0]
        tg = o['vmap'][f[gone]]
        collapsed = (key[f[gone]][:, 0] == key[f[gone]][:, 1]) | (key[f[gone]][:, 1] == key[f[gone]][:, 2]) | \
            (key[f[gone]][:, 0] == key[f[gone]][:, 2])
        assert o['n_survivors'] == len(f) - int(collapsed.sum()) and o['n_duplicates'] == int((~collapsed).sum())
        if (~collapsed).any():
            sets = {tuple(r): i for r, i in zip(map(tuple, np.sort(t, axis=1)), kept)}
            for g, r in zip(gone[~collapsed], np.sort(tg[~collapsed], axis=1)):
                assert sets[tuple(r)] < g                             # the first in input order stayed
        assert np.array_equal(o['verts32'], x.astype(np.float32))


def test_the_restatements_own_error_is_small():
    v, f = mesh_of((24, 20, 18))
    o = S.simplify(v, f, 2.0, with_longdouble=True)
    if np.finfo(np.longdouble).eps < 1e-18:                           # (a platform whose long double is a double has nothing to compare)
        assert 0 < np.abs(o['verts_ld'] - o['verts']).max() < 1e-10


def test_unreferenced_vertices_enter_the_mean_only():
    v = np.array([[0, 0, 0], [2.5, 0, 0], [0, 2.5, 0], [0.5, 0.5, 0.5], [7, 7, 7]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    o = S.simplify(v, f, 1.0, placement='mean', origin=(0, 0, 0))
    assert o['vmap'].tolist() == [0, 2, 1, 0, -1] and o['tris'].tolist() == [[0, 2, 1]]
    assert np.array_equal(o['verts'][0], [0.25, 0.25, 0.25]) and o['m_v'].tolist() == [2, 1, 1]


def test_refused_input_raises():
    v, f = mesh_of((2, 9, 11))
    for cell in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            S.simplify(v, f, cell)
    g = f.copy()
    g[3, 1] = len(v)
    with pytest.raises(ValueError, match='1 triangles'):
        S.simplify(v, g, 1.0)
    w = v.copy()
    w[5, 2] = np.nan
    with pytest.raises(ValueError, match='1 vertices'):
        S.simplify(w, f, 1.0, origin=S.default_origin(v))
    with pytest.raises(ValueError):
        S.simplify(v, f, 1e-7)                                        # an index past 2^21
    o = S.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert o['verts'].shape == (0, 3) and o['tris'].shape == (0, 3)
    o = S.simplify(v[:5], np.zeros((0, 3), np.int32), 1.0)
    assert o['verts'].shape == (0, 3) and o['vmap'].tolist() == [-1] * 5


# ---- the face budget --------------------------------------------------------------------------------------------------------------------
def _first_dip(counts):
    """the first k with n(k) > n(k + 1), None when n is non-decreasing"""
    return next((k for k in range(len(counts) - 1) if counts[k] > counts[k + 1]), None)


# n(k) is NOT monotone on the sphere and on the random field: once the cells are far smaller than the triangles nearly every triangle
# survives and the count wobbles by a few as the grid moves (sphere: n(46) = 15054 > n(47) = 15052; field: n(58) = 97776 > n(59) = 97772).
# Below the first dip it is, and every count behind the dip exceeds every budget below it, so there the bisection must equal the scan.  The
# box replaces them as the case that is monotone over the whole ladder.
@pytest.mark.parametrize('name,budgets,first_dip', [('sphere', (1500, 300, 12000, 15000), 46), ((40, 33, 27), (10000, 2000, 40000, 97000), 58),
                                                    ('box', (100, 1000, 3900, 3980, 5000), None)], ids=str)
def test_bisection_equals_the_linear_scan(name, budgets, first_dip):
    v, f = mesh_of(name)
    counts = S.counts_by_k(v, f)
    assert counts[0] <= 16 and _first_dip(counts) == first_dip
    calls = []

    def n_of_k(k):
        calls.append(k)
        return counts[k]
    for N in budgets:
        assert first_dip is None or N < min(counts[first_dip:])       # the budget lies where n(k) is monotone
        del calls[:]
        k = S.choose_k_bisect(n_of_k, N)
        assert k == S.choose_k_scan(counts, N) and counts[k] <= N and len(calls) <= 8
        assert k == S.K_MAX or counts[k + 1] > N
    with pytest.raises(ValueError):
        S.choose_k_bisect(n_of_k, counts[0] - 1)


def test_cell_table():
    from nero_amd.mesh import simplify_cells
    for D in (1.0, 39.5, 510.99):
        for k in range(81):
            assert simplify_cells(D, k) == S.simplify_cells(D, k)
        assert simplify_cells(D, 0) == D and simplify_cells(D, 8) == D / 4 and simplify_cells(D, 80) == D / 2 ** 20
    assert abs(S.CELL_FACTORS[1] - 2 ** -0.25) < 1e-16 and abs(S.CELL_FACTORS[3] - 2 ** -0.75) < 1e-16
    for bad in (-1, 81):
        with pytest.raises(ValueError):
            simplify_cells(1.0, bad)


# ---- the C surface ----------------------------------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib as L
    return L.bind(C.CDLL(os.path.join(ROOT, 'nero_amd', 'libnero_hip.so')))


def test_symbols_exist_and_are_declared():
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'nero_hip.h')).read()
    for name in ('nero_mesh_simplify_workspace_bytes', 'nero_mesh_simplify_count', 'nero_mesh_simplify_emit'):
        assert hasattr(lib, name) and name + '(' in hdr, name


def test_workspace_is_monotone_and_refuses_sizes_out_of_range():
    ws = _lib().nero_mesh_simplify_workspace_bytes
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4095, 4096, 4097, 10 ** 5, 10 ** 6, 3 * 10 ** 6, 2 ** 24, 2 ** 27,
             (2 ** 31 - 1) // 3]
    assert ws(0, 0) > 0
    for T in sizes:
        row = [ws(V, T) for V in sizes + [2 ** 31 - 1]]
        assert all(0 < a <= b for a, b in zip(row[:-1], row[1:])), (T, row)
    for V in sizes:
        col = [ws(V, T) for T in sizes]
        assert all(0 < a <= b for a, b in zip(col[:-1], col[1:])), (V, col)
    assert ws(10 ** 6, 2 * 10 ** 6) >= 10 ** 6 * 56 + 2 * 10 ** 6 * 100  # every array the passes keep, beside the scratch
    for V, T in ((-1, 0), (0, -1), (2 ** 31, 0), (0, (2 ** 31 - 1) // 3 + 1), (-2 ** 40, -2 ** 40)):
        assert ws(V, T) == 0


def test_refused_arguments_give_error_codes_without_a_device():
    """every check below is made before the first HIP call"""
    lib = _lib()
    ARG, UNSUPPORTED = -1, -3
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    count = lambda **k: lib.nero_mesh_simplify_count(k.get('verts', p), k.get('tris', p), k.get('T', 4), k.get('V', 4), k.get('cell', 1.0),
                                                     k.get('origin', origin), 0, k.get('ws', p), k.get('totals', p), None)
    emit = lambda **k: lib.nero_mesh_simplify_emit(k.get('verts', p), k.get('tris', p), k.get('T', 4), k.get('V', 4), k.get('cell', 1.0),
                                                   k.get('origin', origin), k.get('placement', 1), 1, k.get('ws', p), p, p, p,
                                                   k.get('v_cap', 4), p, k.get('t_cap', 4), None, None, None, None)
    nan_origin = (C.c_double * 3)(0.0, float('nan'), 0.0)
    for call in (count, emit):
        for null in ('verts', 'tris', 'ws', 'origin'):
            assert call(**{null: None}) == ARG and b'nero_mesh_simplify' in lib.nero_last_error(), null
        for cell in (0.0, -2.0, float('nan'), float('inf')):
            assert call(cell=cell) == ARG and b'cell' in lib.nero_last_error()
        assert call(origin=nan_origin) == ARG
        for sizes in ({'V': -1}, {'T': -1}, {'V': 2 ** 31}, {'T': (2 ** 31 - 1) // 3 + 1}):
            assert call(**sizes) == UNSUPPORTED, sizes
    assert count(totals=None) == ARG
    assert emit(placement=2) == ARG and emit(placement=-1) == ARG
    assert emit(v_cap=-1) == ARG and emit(t_cap=-1) == ARG


# ---- hand-offs --------------------------------------------------------------------------------------------------------------------------
def test_simple_atlas_takes_the_simplified_sphere():
    from nero_amd.texture import simple_atlas
    v, f = mesh_of('sphere')
    with pytest.raises(ValueError):
        simple_atlas(v, f, 256)
    o = S.simplify(v, f, 4.0)
    vt, ft = simple_atlas(o['verts32'], o['tris'], 256)
    assert ft.shape == o['tris'].shape and vt.shape == (3 * len(ft), 2) and 0 < len(ft) <= 2 * (256 // 4) ** 2


def test_extract_geometry_signature():
    from nero_amd.renderer import NeROShapeRenderer
    params = list(inspect.signature(NeROShapeRenderer.extract_geometry).parameters.values())
    assert params[-1].name == 'simplify' and params[-1].default is None and params[-2].name == 'clean'


def test_python_argument_checks_need_no_device():
    from nero_amd import mesh as M
    assert M.SIMPLIFY_FACTORS == S.CELL_FACTORS and M.SIMPLIFY_K_MAX == S.K_MAX
    with pytest.raises(TypeError):
        M.simplify_mesh_device(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), cell=1.0)


def test_script_command_line():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import extract_mesh as E
    finally:
        sys.path.pop(0)
    a = E.parse_args(['--in', 'a.ply', '--out', 'b.ply', '--target-faces', '1500'])
    assert E.simplify_of(a) == {'target_faces': 1500} and E.rules_of(a) is None
    a = E.parse_args(['--cfg', 'c.yaml', '--out', 'b.ply', '--keep-largest', '--simplify-cell', '2.5'])
    assert E.simplify_of(a) == {'cell': 2.5} and E.rules_of(a) == {'keep': 1}
    assert E.simplify_of(E.parse_args(['--in', 'a.ply', '--out', 'b.ply'])) is None
    with pytest.raises(SystemExit):
        E.parse_args(['--in', 'a.ply', '--out', 'b.ply', '--target-faces', '10', '--simplify-cell', '2'])
