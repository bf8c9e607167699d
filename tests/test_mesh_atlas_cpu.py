"""CPU tier: the numpy restatement of the projection atlas (tests/mesh_atlas_ref.py) pinned to the counts measured with the
definition, its invariants (every face that can have a chart has one, charts connected and of one class, positive UV areas), the packing
and the scale search (also the host packing of nero_amd.texture against the restatement), and what the atlas covers under the raster's rule
(tests/texture_ref.py): charts inside their rectangles, `gutter` texels apart, no texel covered twice unless a chart folds over itself."""
import numpy as np
import pytest

from tests import mesh_atlas_ref as A
from tests import texture_ref as TR

# fixture -> (charts, chartless faces, boundary edges); no fixture has a non-manifold edge
COUNTS = {'sphere': (6, 0, 0), 'torus': (21, 0, 0), 'two_spheres': (12, 0, 0), 'tube': (45, 0, 0), (24, 20, 18): (7262, 852, 2288),
          (40, 33, 27): (30923, 4059, 6178), (2, 9, 11): (129, 8, 203)}
GUTTER = 4


def _size(name):
    return A.SIZE.get(name, 128)


def _interior_edges(c):
    """(t, n) with t < n for every edge two faces share"""
    T = len(c['nbr'])
    t = np.repeat(np.arange(T), 3)
    n = c['nbr'].reshape(-1).astype(np.int64)
    keep = (n >= 0) & (t < n)
    return t[keep], n[keep]


@pytest.mark.parametrize('name', A.FIXTURES, ids=str)
def test_chart_counts_are_the_measured_ones(name):
    v, f = A.mesh_of(name)
    c = A.ref_charts(name)
    assert (c['K'], c['chartless'], c['boundary']) == COUNTS[name] and c['nonmanifold'] == 0
    assert c['n_faces'].sum() == len(f) - c['chartless'] and (c['n_faces'] > 0).all()
    assert np.array_equal(np.unique(c['chart'][c['chart'] >= 0]), np.arange(c['K']))
    first = np.full(c['K'], len(f))
    np.minimum.at(first, c['chart'][c['chart'] >= 0], np.nonzero(c['chart'] >= 0)[0])
    assert np.all(np.diff(first) > 0)                                # numbered by ascending smallest face


def test_the_sphere_has_few_seams():
    c = A.ref_charts('sphere')
    t, n = _interior_edges(c)
    seams = int((c['chart'][t] != c['chart'][n]).sum())
    print(f'sphere: {seams} seams among {len(t)} interior edges')
    assert len(t) == 22638 and seams <= 0.05 * len(t)


@pytest.mark.parametrize('name', A.FIXTURES + ['box', 'ramp'], ids=str)
def test_every_face_that_can_have_a_chart_has_one_and_charts_are_connected_and_of_one_class(name):
    v, f = A.mesh_of(name)
    c = A.ref_charts(name)
    p = v.astype(np.float64)
    ok = A.valid_faces(f, len(v))
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    can = ok & np.isfinite(n).all(1) & (n != 0).any(1)
    assert np.array_equal(c['chart'] >= 0, can)
    # no face of a fixture projects with zero or negative area: the component along the dominant axis, signed by the class, is positive
    k = c['face_class'][can] >> 1
    sgn = np.where(c['face_class'][can] & 1, -1.0, 1.0)
    assert (sgn * n[can][np.arange(can.sum()), k] > 0).all()
    assert (c['chart_class'][c['chart'][can]] == c['face_class'][can]).all()                  # one class per chart
    # connected: labels spread over the joins (same chart across a shared edge) by repeated minima reach one value per chart
    t, m = _interior_edges(c)
    same = c['chart'][t] == c['chart'][m]
    t, m = t[same & (c['chart'][t] >= 0)], m[same & (c['chart'][t] >= 0)]
    lab = np.arange(len(f))
    for _ in range(len(f)):
        new = lab.copy()
        np.minimum.at(new, t, lab[m])
        np.minimum.at(new, m, lab[t])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    assert len(np.unique(lab[can])) == c['K']
    # and two charts never share an edge between faces of one class (they would be one chart)
    t, m = _interior_edges(c)
    cut = c['chart'][t] != c['chart'][m]
    assert (c['face_class'][t[cut]] != c['face_class'][m[cut]]).all()


@pytest.mark.parametrize('name', A.FIXTURES + ['box', 'ramp'], ids=str)
def test_uv_triangles_of_charted_faces_have_positive_area(name):
    r = A.ref_atlas(name, _size(name), GUTTER)
    assert r['scale'] > 0
    uv = r['vt'].astype(np.float64)[r['ft']]
    a = (uv[:, 1, 0] - uv[:, 0, 0]) * (uv[:, 2, 1] - uv[:, 0, 1]) - (uv[:, 2, 0] - uv[:, 0, 0]) * (uv[:, 1, 1] - uv[:, 0, 1])
    has = r['chart'] >= 0
    assert (a[has] > 0).all()
    assert (a[~has] == 0).all() and (r['ft'][~has] == len(r['vt']) - 1).all()
    if (~has).any():
        assert r['vt_vertex'][-1] == -1 and r['vt_chart'][-1] == -1 and (r['vt'][-1] == 0).all()
    assert (r['vt_vertex'][:len(r['vt']) - int((~has).any())] >= 0).all()
    key = r['vt_chart'].astype(np.int64)[:len(r['vt']) - int((~has).any())] << 32 | r['vt_vertex'][:len(r['vt']) - int((~has).any())]
    assert np.all(np.diff(key) > 0)                                  # ascending (chart, vertex), each pair once
    _, f = A.mesh_of(name)
    assert np.array_equal(r['vt_vertex'][r['ft'][has]], f[has])      # vmapping: the UV vertex of a corner is a copy of that corner's vertex
    assert np.array_equal(r['vt_chart'][r['ft'][has]], np.repeat(r['chart'][has][:, None], 3, 1))


# ---- packing ----------------------------------------------------------------------------------------------------------------------------
def _assert_packed(rects, size, gutter):
    m = gutter // 2
    x0, y0, x1, y1 = rects[:, 0], rects[:, 1], rects[:, 0] + rects[:, 2], rects[:, 1] + rects[:, 3]
    assert (x0 >= m).all() and (y0 >= m).all() and (x1 <= size - m).all() and (y1 <= size - m).all()
    # empty texels between two rectangles along the axis where they are farther apart: at least `gutter`
    gx = np.maximum(x0[:, None] - x1[None, :], x0[None, :] - x1[:, None])
    gy = np.maximum(y0[:, None] - y1[None, :], y0[None, :] - y1[:, None])
    gap = np.maximum(gx, gy)
    np.fill_diagonal(gap, gutter)
    assert gap.min() >= gutter


@pytest.mark.parametrize('name,size,gutter', [('sphere', 128, 4), ('torus', 64, 4), ('tube', 128, 5), ((2, 9, 11), 128, 4), ((24, 20, 18), 512, 1),
                                              ('box', 64, 0), ('tube', 256, 8)], ids=str)
def test_rectangles_keep_the_gutter_and_the_margin_and_the_bisection_fits(name, size, gutter):
    c = A.ref_charts(name)
    scale, rects, steps = A.choose_scale(c['box'], size, gutter)
    ep, eq = A.extents(c['box'])
    assert np.array_equal(rects[:, 2], np.ceil(ep * scale) + 1) and np.array_equal(rects[:, 3], np.ceil(eq * scale) + 1)
    if len(rects) <= 2000:
        _assert_packed(rects, size, gutter)
    hi = (size - 2 * (gutter // 2) - 1) / max(ep.max(), eq.max())
    if A.pack(c['box'], hi, size, gutter) is None:
        assert steps == 32 and 0 <= scale < hi and A.pack(c['box'], scale, size, gutter) is not None
    else:
        assert steps == 0 and scale == hi
    r2 = A.choose_scale(c['box'], size, gutter)
    assert r2[0] == scale and np.array_equal(r2[1], rects)           # deterministic


def test_the_host_packing_of_the_package_is_the_restatement():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import texture as TX
    for name, size, gutter in [('sphere', 128, 4), ('tube', 64, 3), ((2, 9, 11), 64, 4), ((2, 9, 11), 128, 4), ((24, 20, 18), 512, 2), ('ramp', 64, 4)]:
        c = A.ref_charts(name)
        want = A.choose_scale(c['box'], size, gutter)
        got = TX.choose_scale(c['box'], size, gutter)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2], (name, size, gutter)
        for s in (0.0, 0.37 * want[0], want[0], 1.5 * want[0] + 0.1, 1e9, np.inf, np.nan):
            a, b = A.pack(c['box'], s, size, gutter), TX.pack_charts(c['box'], s, size, gutter)
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (name, size, gutter, s)


def test_value_errors_of_the_scale_search():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import texture as TX
    c = A.ref_charts('tube')                                         # 45 charts
    for mod in (A, TX):
        s, rects, steps = mod.choose_scale(c['box'], 128, 4, texels_per_unit=0.25)
        assert s == 0.25 and steps == 0 and len(rects) == 45
        with pytest.raises(ValueError):
            mod.choose_scale(c['box'], 128, 4, texels_per_unit=50.0)
        with pytest.raises(ValueError, match=r'\b27\b'):             # 7 x 7 cells: 7 + 6 gutters of 3 + the margins 1 + 1
            mod.choose_scale(c['box'], 20, 3)
        s, rects, _ = mod.choose_scale(c['box'], 27, 3)              # ... and at 27 every chart is one texel
        assert s == 0.0 and (rects[:, 2:] == 1).all()
    assert A.min_size(45, 3) == 27 and A.min_size(1, 4) == 5 and A.min_size(0, 4) == 1
    s, rects, steps = A.choose_scale(np.zeros((0, 4), np.float32), 16, 4)  # no chart at all
    assert s == 1.0 and rects.shape == (0, 4) and steps == 0
    s, rects, _ = A.choose_scale(np.zeros((3, 4), np.float32), 16, 4)       # charts without extent: scale 1, one texel each
    assert s == 1.0 and (rects[:, 2:] == 1).all()


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,size', [('sphere', 64), ('sphere', 128), ('torus', 64), ('torus', 128), ('box', 64), ('box', 128), ('tube', 128),
                                       ((2, 9, 11), 128)], ids=str)
def test_charts_cover_their_own_rectangles_a_gutter_apart_and_nothing_twice(name, size):
    r = A.ref_atlas(name, size, GUTTER)
    tri_id, cover = TR.raster(r['vt'], r['ft'], size, size, count=True)
    assert (tri_id >= 0).sum() > 0.1 * size * size * r['fill']
    A.assert_gutter_and_containment(A.chart_map(tri_id, r['chart']), r['rects'], GUTTER)
    assert int((cover > 1).sum()) == 0
    if (r['chart'] < 0).any():
        assert not np.isin(tri_id, np.nonzero(r['chart'] < 0)[0]).any()      # a chartless face covers nothing


def test_a_helical_ramp_overlaps_itself_and_the_count_is_the_brute_force_one():
    v, f = A.mesh_of('ramp')
    r = A.ref_atlas('ramp', 64, GUTTER)
    assert r['K'] == 1 and (r['face_class'] == 4).all()              # one chart: every face looks up and all are joined
    _, cover = TR.raster(r['vt'], r['ft'], 64, 64, count=True)
    n = int((cover > 1).sum())
    assert n > 100 and n == A.overlap_brute(r['vt'], r['ft'], 64, 64)
