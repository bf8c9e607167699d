"""CPU tier of the closest-point query (include/nero_closest.h, nero_amd/csrc/closest_point_math.h) on the numpy
restatement tests/closest_ref.py:
  * the kernel's walk -- its padded box bound, its order of visits -- returns in float32 what exhaustive search returns, bit for bit, on every
    mesh of tests/tracer_ref.py and every query set; with the pad set to zero it does not;
  * float32 against float64: the gap is measured, reported, and held to the bounds derived from the operation count;
  * the arithmetic header itself, compiled for the host as a stand-alone program under the sanitizers, prints the restatement's bits;
  * the header is bound from the second list of nero_amd/_lib.py, and the entry point refuses bad arguments before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import closest_ref as CR
from tests import tracer_ref as TR
from tests.helpers import parity_report, run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
ILL = ('slivers', 'degenerate')               # meshes on which only the conditions that do not depend on conditioning are asserted
FIELDS = ('d2', 'face', 'b1', 'b2', 'slot')


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _differ(a, b):
    """per point: does any field differ, floats compared as bits"""
    return np.any([_bits(a[k]) != _bits(b[k]) for k in FIELDS], axis=0)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib
    return _lib


# ---- the walk against exhaustive search ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TR.MESHES)
def test_the_walk_equals_exhaustive_search_bit_for_bit(name):
    tree = TR.tree(name)
    for which in CR.SETS:
        pts = CR.query_set(name, which)
        assert pts.shape == (CR.N_POINTS, 3)
        want = CR.reference(name, which)
        got = CR.walk(pts, tree)
        bad = _differ(got, want)
        assert not bad.any(), f'{name}, {which}: {int(bad.sum())} of {len(pts)} points differ from exhaustive search, first {int(np.argmax(bad))}'
        assert (want['face'] >= 0).all() and np.isfinite(want['d2']).all()
        if name in ('hf_smooth', 'hf_noisy', 'mc_sphere', 'box') and which != 'origin':      # the walk is a walk: it leaves most of the tree unread
            assert got['visits'].mean() < tree['info'][0] / 2, (name, which, float(got['visits'].mean()), tree['info'][0])


def test_ties_are_the_normal_case_and_go_to_the_lowest_face():
    """a query on a mesh vertex is equally near to every incident face: several triangles attain the minimum, and the lowest face is reported"""
    for name in ('hf_noisy', 'box', 'mc_sphere'):
        tree, pts, want = TR.tree(name), CR.query_set(name, 'vertex'), CR.reference(name, 'vertex')
        v0, e1, e2 = CR._records(tree['tri_array'], np.float32)
        d2 = CR.point_triangle(pts[:50, None, :], v0[None], e1[None], e2[None])[0]
        ties = (d2 == want['d2'][:50, None])
        assert (ties.sum(1) >= 2).mean() > 0.9, name
        order = np.asarray(tree['order'])
        assert np.array_equal(want['face'][:50], np.where(ties, order[None, :], np.iinfo(np.int64).max).min(1))


def test_without_the_pad_the_walk_does_not_equal_exhaustive_search():
    """the same comparison with CP_PAD = 0 fails: on the 'far' set the computed bound of a box exceeds the computed d2 of a triangle inside it,
    and a subtree that holds the answer (or an equally near triangle of a lower face) is pruned"""
    wrong = {}
    for name in ('hf_noisy', 'box'):
        pts = CR.query_set(name, 'far')
        assert np.abs(pts).max() > 4
        wrong[name] = int(_differ(CR.walk(pts, TR.tree(name), pad=0.0), CR.reference(name, 'far')).sum())
        assert not _differ(CR.walk(pts, TR.tree(name)), CR.reference(name, 'far')).any()
    print('points of the far set the unpadded walk gets wrong:', wrong)
    assert all(n >= 1 for n in wrong.values()), wrong


def test_max_dist_and_points_out_of_range():
    name = 'hf_noisy'
    tree, pts, want = TR.tree(name), CR.query_set(name, 'off_0.1'), CR.reference(name, 'off_0.1')
    r2 = np.sort(want['d2'])[len(pts) // 2]
    near = want['d2'] <= r2
    assert near.any() and not near.all() and (want['d2'] == r2).any()           # a point AT d2 == r2 is found
    for res in (CR.walk(pts, tree, r2=r2), CR.exhaustive(pts, tree['tri_array'], tree['order'], r2=r2)):
        assert np.array_equal(res['face'] >= 0, near)
        assert not _differ({k: v[near] for k, v in res.items()}, {k: v[near] for k, v in want.items()}).any()
        assert np.all(np.isinf(res['d2'][~near])) and np.all(res['b1'][~near] == 0) and np.all(res['b2'][~near] == 0)


# ---- float32 against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TR.MESHES)
def test_float32_against_float64(name):
    """dist32 = sqrt(d2) of the float32 restatement, dist64 the same formulation in float64 on the same stored triangles.  With u = 2^-24 and
    D = the distance from the point to the farthest corner of the mesh's bounding box (DESIGN.md 9.13.2 has the derivation):
      * below:  dist32 >= dist64 - EVAL u D, on every mesh: d2 belongs to a point OF some triangle, which is no nearer than the surface, and
        evaluating it costs at most EVAL = 10 roundings of size u D;
      * above, well-shaped meshes:  dist32 <= dist64 + (EVAL + max(EDGE, interior_factor(s))) u D, s the sine of the angle at v0 of the triangle
        float64 finds: the float32 run evaluates that triangle too, and its candidate for the same feature lies within EDGE u D (an edge
        segment) or interior_factor(s) u D (the foot of the perpendicular) of the float64 one;
      * above, every mesh, and the only upper bound on slivers and degenerate:  dist32 <= dist64 + inradius + (EVAL + EDGE) u D of that
        triangle: the edge candidates are always there, and no point of a triangle is farther than the inradius from its boundary (a zero-area triangle has inradius 0, so the rounding
        term has to stand beside it).
    Measured (this file, printed and reported): |gap| <= 1.7 u D on the well-shaped meshes against bounds of 24 u D (edge) to ~100 u D
    (interior, s ~ 0.7) -- the derived bounds are 15 to 60 times the measurement and are kept as derived."""
    tree = TR.tree(name)
    worst = {}
    for which in CR.SETS:
        pts = CR.query_set(name, which)
        r32, r64 = CR.reference(name, which), CR.reference(name, which, 'float64')
        assert r32['d2'].dtype == np.float32 and r64['d2'].dtype == np.float64
        d32, d64 = np.sqrt(r32['d2'].astype(np.float64)), np.sqrt(r64['d2'])
        uD = CR.U * CR.scale(pts, tree['tri_array'])
        sine, inradius = CR.triangle_shape(tree['tri_array'], r64['slot'])
        gap = d32 - d64
        worst[which] = (float(gap.min()), float(gap.max()), float((gap / uD).min()), float((gap / uD).max()))
        # conditions that hold whatever the conditioning
        assert np.isfinite(r32['d2']).all() and np.isfinite(r32['b1']).all() and np.isfinite(r32['b2']).all(), (name, which)
        b1, b2 = r32['b1'].astype(np.float64), r32['b2'].astype(np.float64)
        assert (b1 >= 0).all() and (b2 >= 0).all() and (b1 + b2 <= 1).all(), (name, which)
        assert (gap >= -CR.EVAL * uD).all(), (name, which, worst[which])
        assert (gap <= inradius + (CR.EVAL + CR.EDGE) * uD).all(), (name, which, worst[which])
        if name not in ILL:
            with np.errstate(divide='ignore'):
                above = (CR.EVAL + np.maximum(CR.EDGE, CR.interior_factor(sine))) * uD
            assert (gap <= above).all(), (name, which, worst[which], float((gap / above).max()))
    print(name, worst)
    parity_report(f'test_closest_point_cpu::float32_against_float64[{name}]', file='closest_point_gaps.json',
                  gap_min_max_and_in_units_of_uD={k: [float(f'{x:.3e}') for x in v] for k, v in worst.items()})


# ---- the header's own arithmetic, on the host, under the sanitizers ------------------------------------------------------------------------
def test_the_header_on_the_host_prints_the_bits_of_the_restatement(tmp_path):
    """tests/closest_point_main.cpp includes nero_amd/csrc/closest_point_math.h -- the source the kernel compiles -- and runs under
    address,undefined (tests.helpers.run_host_program; the only sanitizer run of this feature: nothing loaded into Python is sanitized)"""
    out = run_host_program(tmp_path, 'closest_point_main.cpp', extra=('-ffp-contract=off',))
    rows = np.array([[float.fromhex(x) for x in ln.split()] for ln in out.splitlines()], np.float64)
    assert rows.shape[1] == 23 and len(rows) >= 100
    f = rows.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), rows)                # every printed number is a float32
    p, v0, e1, e2, mn, mx = (f[:, 3 * k:3 * k + 3] for k in range(6))
    d2, b1, b2 = CR.point_triangle(p, v0, e1, e2)
    for got, want, what in ((f[:, 18], d2, 'd2'), (f[:, 19], b1, 'b1'), (f[:, 20], b2, 'b2'),
                            (f[:, 21], CR.box_bound(mn, mx, p, CR.CP_PAD), 'padded bound'), (f[:, 22], CR.box_bound(mn, mx, p, 0.0), 'bare bound')):
        bad = got.view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)
        assert want.dtype == np.float32 and not bad.any(), f'{what}: {int(bad.sum())} rows differ, first {int(np.argmax(bad))}'
    # the table holds what it has to hold
    area = np.linalg.norm(np.cross(e1.astype(np.float64), e2.astype(np.float64)), axis=1)
    d = p.astype(np.float64) - v0
    on_vertex = (d == 0).all(1) | (d == e1).all(1) | (d == e2).all(1)
    on_edge = (np.abs(d - 0.5 * e1.astype(np.float64)) <= 1e-6).all(1) & ~on_vertex
    in_plane = (np.abs((d * np.cross(e1.astype(np.float64), e2.astype(np.float64))).sum(1)) <= 1e-6 * area) & (area > 0)
    assert (area == 0).sum() >= 40 and on_vertex.sum() >= 20 and on_edge.sum() >= 5 and (in_plane & ~on_vertex & ~on_edge).sum() >= 10
    assert np.isfinite(f[:, 18:21]).all() and (f[on_vertex, 18] == 0).all()
    assert (f[:, 19] >= 0).all() and (f[:, 20] >= 0).all() and (rows[:, 19] + rows[:, 20] <= 1).all()
    assert (f[:, 21] <= f[:, 22]).all() and (f[:, 21] <= f[:, 18]).all()        # the padded bound of a triangle's own box never exceeds its d2


# ---- the binding, on the second list ------------------------------------------------------------------------------------------------------
def test_the_header_is_bound_from_the_second_list(L):
    assert [os.path.basename(h) for h in L.EXTRA_HEADER_PATHS] == ['nero_closest.h']
    assert not set(L.EXTRA_HEADER_PATHS) & set(L.HEADER_PATHS)
    assert all(os.path.dirname(h) == os.path.dirname(L.HEADER_PATH) and not os.path.basename(h).startswith('nero_hip') for h in L.EXTRA_HEADER_PATHS)
    both = L.parse_headers(L.HEADER_PATHS + L.EXTRA_HEADER_PATHS)                  # (a name declared twice would raise)
    extra = L.parse_headers(L.EXTRA_HEADER_PATHS)
    assert len(both) == len(L.parse_headers()) + len(extra) and set(extra) == {'nero_bvh_closest'}
    assert both['nero_bvh_closest'][2] == 'nero_closest.h'
    p, f, i, i64 = C.c_void_p, C.c_float, C.c_int, C.c_int64
    for lib in (L.lib, L.bind(L.bind(C.CDLL(L.LIB_PATH)), L.EXTRA_HEADER_PATHS)):
        fn = lib.nero_bvh_closest
        assert fn.restype is i and fn.argtypes == [p, p, i64, f, p, p, p, p, p]
    assert C.CDLL(L.LIB_PATH).nero_bvh_closest.argtypes is None      # a bare handle knows nothing: the types come from the header alone


def test_a_newer_closest_header_makes_the_library_stale(L):
    import __graft_entry__ as ge
    assert not ge.library_is_stale()
    path = L.EXTRA_HEADER_PATHS[0]
    st = os.stat(path)
    try:
        os.utime(path, ns=(st.st_atime_ns, os.stat(ge.LIB).st_mtime_ns + 10 ** 9))
        assert ge.library_is_stale()
    finally:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not ge.library_is_stale()


def test_the_entry_point_refuses_bad_arguments_without_a_device(L):
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    inf = float('inf')
    for k in (0, 1, 4, 5):                                            # handle, pts, dist, face
        a = [p, p, 4, inf, p, p, p, p, None]
        a[k] = None
        assert lib.nero_bvh_closest(*a) == ERR_ARG and 'nero_bvh_closest' in err() and 'null' in err()
    assert lib.nero_bvh_closest(p, p, -1, inf, p, p, p, p, None) == ERR_ARG and 'n must be' in err()
    assert lib.nero_bvh_closest(p, p, 2 ** 36 + 1, inf, p, p, p, p, None) == ERR_ARG and '2^36' in err()
    for bad in (0.0, -0.0, -1.0, -inf, float('nan')):
        assert lib.nero_bvh_closest(p, p, 4, bad, p, p, None, None, None) == ERR_ARG and 'max_dist' in err()
        assert lib.nero_bvh_closest(p, p, 0, bad, p, p, None, None, None) == ERR_ARG          # before n == 0 is looked at
    # n = 0 with valid arguments: nothing to do, no device needed; the optional outputs may be absent
    assert lib.nero_bvh_closest(p, p, 0, inf, p, p, None, None, None) == 0
    assert lib.nero_bvh_closest(p, p, 0, 0.5, p, p, p, p, None) == 0
