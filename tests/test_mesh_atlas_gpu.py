"""GPU tier: the projection atlas (nero_amd/csrc/mesh_atlas.hip, nero_uv_overlap_count of texture.hip) through the C ABI and through
nero_amd.mesh / nero_amd.texture against the numpy restatement tests/mesh_atlas_ref.py: exact agreement of every integer output, bit-equal
UVs, the smallest shapes at which each step can go wrong, guards round every output, determinism, renumbering, the coverage properties
through the device raster, the bake with atlas='charts' end to end, and scripts/extract_texture_maps.py --atlas charts."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import mesh_atlas_ref as A
from tests import texture_ref as TR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUTTER = 4
PAD = 64                                                             # guard words on either side of every output
GUARD = 0x5A5A5A5A
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _dev(v, f):
    return (torch.from_numpy(np.array(v, np.float32)).cuda().reshape(-1, 3), torch.from_numpy(np.array(f, np.int32)).cuda().reshape(-1, 3))


def _eq(t, a):
    a = np.ascontiguousarray(a)
    return tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


def _bits(t, a):
    """float32 outputs compared as bits"""
    return _eq(t.contiguous().view(torch.int32), np.ascontiguousarray(a, dtype=np.float32).view(np.int32))


class Guarded:
    """n 4-byte words (or n 8-byte words) between two runs of guard words"""

    def __init__(self, n, dtype):
        self.words = n * (2 if dtype == torch.int64 else 1)
        self.buf = torch.full((self.words + 2 * PAD,), GUARD, dtype=torch.int32, device='cuda')
        self.dtype, self.n = dtype, n

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def get(self):
        return self.buf[PAD:PAD + self.words].view(self.dtype).cpu().numpy()

    def guards_intact(self):
        return bool((self.buf[:PAD] == GUARD).all()) and bool((self.buf[PAD + self.words:] == GUARD).all())

    def untouched(self):
        return bool((self.buf == GUARD).all())


def cabi_atlas(v, f, size, gutter, vt_cap=None):
    """every entry point of the atlas through ctypes with guarded outputs -> dict of host arrays (rc of the emit under 'emit_rc')"""
    from nero_amd import _lib as L
    lib = L.lib
    vd, fd = _dev(v, f)
    V, T = vd.shape[0], fd.shape[0]
    s = L.stream_ptr()
    p = lambda t: t.data_ptr() if t.numel() else None
    ws = lambda n: torch.empty(max(int(n), 256), dtype=torch.uint8, device='cuda')
    out, g = {}, {}
    g['nbr'], g['counts'] = Guarded(3 * T, torch.int32), Guarded(2, torch.int64)
    w = ws(lib.nero_mesh_face_adjacency_workspace_bytes(T))
    L.check(lib.nero_mesh_face_adjacency(p(fd), T, V, w.data_ptr(), g['nbr'].ptr, g['counts'].ptr, s))
    g['face_class'], g['chart'], g['info'] = Guarded(T, torch.int32), Guarded(T, torch.int32), Guarded(2, torch.int64)
    w = ws(lib.nero_mesh_chart_label_workspace_bytes(T))
    L.check(lib.nero_mesh_chart_label(p(vd), p(fd), T, V, g['nbr'].ptr, w.data_ptr(), g['face_class'].ptr, g['chart'].ptr, g['info'].ptr, s))
    K, chartless = (int(x) for x in g['info'].get())
    g['chart_class'], g['n_faces'], g['box'] = Guarded(K, torch.int32), Guarded(K, torch.int32), Guarded(4 * K, torch.float32)
    L.check(lib.nero_mesh_chart_stats(p(vd), p(fd), T, V, g['chart'].ptr, g['face_class'].ptr, K, g['chart_class'].ptr, g['n_faces'].ptr,
                                      g['box'].ptr, s))
    g['totals'] = Guarded(2, torch.int64)
    w = ws(lib.nero_mesh_chart_corners_workspace_bytes(T))
    L.check(lib.nero_mesh_chart_corners_count(p(fd), T, V, g['chart'].ptr, K, w.data_ptr(), g['totals'].ptr, s))
    n_vt, chartless_corners = (int(x) for x in g['totals'].get())
    assert chartless_corners == 3 * chartless
    cap = n_vt if vt_cap is None else vt_cap
    g['ft'], g['vt_vertex'], g['vt_chart'] = Guarded(3 * T, torch.int32), Guarded(cap, torch.int32), Guarded(cap, torch.int32)
    out['emit_rc'] = lib.nero_mesh_chart_corners_emit(T, w.data_ptr(), g['ft'].ptr, g['vt_vertex'].ptr, g['vt_chart'].ptr, cap, s)
    out['guards'] = g
    out.update(K=K, chartless=chartless, n_vt=n_vt)
    if out['emit_rc'] == 0:
        box = g['box'].get().reshape(K, 4)
        scale, rects, _ = A.choose_scale(box, size, gutter)
        origin = torch.from_numpy(np.ascontiguousarray(rects[:, :2], dtype=np.int32)).cuda()
        g['vt'] = Guarded(2 * n_vt, torch.float32)
        L.check(lib.nero_mesh_chart_uv(p(vd), V, g['vt_vertex'].ptr, g['vt_chart'].ptr, n_vt, g['chart_class'].ptr, g['box'].ptr, p(origin), K,
                                       float(scale), size, g['vt'].ptr, s))
        out.update(scale=scale, rects=rects)
    torch.cuda.synchronize()
    for k, x in g.items():
        assert x.guards_intact(), k
        out[k] = x.get()
    return out


def assert_cabi_equals(o, r, T):
    assert o['emit_rc'] == 0
    assert np.array_equal(o['nbr'].reshape(T, 3), r['nbr']) and o['counts'].tolist() == [r['boundary'], r['nonmanifold']]
    assert np.array_equal(o['face_class'], r['face_class']) and np.array_equal(o['chart'], r['chart'])
    assert (o['K'], o['chartless']) == (r['K'], r['chartless'])
    assert np.array_equal(o['chart_class'], r['chart_class']) and np.array_equal(o['n_faces'], r['n_faces'])
    assert np.array_equal(o['box'].view(np.int32).reshape(-1, 4), r['box'].view(np.int32))
    assert np.array_equal(o['ft'].reshape(T, 3), r['ft']) and np.array_equal(o['vt_vertex'], r['vt_vertex'])
    assert np.array_equal(o['vt_chart'], r['vt_chart'])
    assert o['scale'] == r['scale'] and np.array_equal(o['rects'], r['rects'])
    assert np.array_equal(o['vt'].view(np.int32).reshape(-1, 2), r['vt'].view(np.int32))


def assert_api_equals(v, f, r, size, gutter=GUTTER):
    from nero_amd import mesh as M
    from nero_amd import texture as TX
    vd, fd = _dev(v, f)
    nbr, nb, nm = M.face_adjacency_device(fd, vd.shape[0])
    assert _eq(nbr, r['nbr']) and (nb, nm) == (r['boundary'], r['nonmanifold'])
    chart, cls, nbr2, ci = M.face_charts_device(vd, fd)
    assert chart.dtype == cls.dtype == nbr2.dtype == torch.int32 and _eq(chart, r['chart']) and _eq(cls, r['face_class']) and _eq(nbr2, r['nbr'])
    assert (ci.K, ci.n_chartless, ci.n_boundary, ci.n_nonmanifold) == (r['K'], r['chartless'], r['boundary'], r['nonmanifold'])
    assert _eq(ci.chart_class, r['chart_class']) and _eq(ci.n_faces, r['n_faces']) and _bits(ci.box, r['box'])
    vt, ft, info = TX.chart_atlas(vd, fd, size, gutter)
    assert vt.is_cuda and ft.is_cuda and vt.dtype == torch.float32 and ft.dtype == torch.int32
    assert _eq(ft, r['ft']) and _eq(info.vt_vertex, r['vt_vertex']) and _eq(info.vt_chart, r['vt_chart']) and _eq(info.chart, r['chart'])
    assert info.scale == r['scale'] and np.array_equal(info.rects, r['rects']) and info.n_charts == r['K']
    assert info.bisection_steps == r['steps'] and info.fill == r['fill']
    assert _bits(vt, r['vt'])
    return vt, ft, info


# ---- agreement on the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', A.FIXTURES + ['box', 'ramp'], ids=str)
def test_the_atlas_equals_the_restatement_on_every_fixture(name):
    v, f = A.mesh_of(name)
    size = A.SIZE.get(name, 128)
    r = A.ref_atlas(name, size, GUTTER)
    assert_api_equals(v, f, r, size)
    assert_cabi_equals(cabi_atlas(v, f, size, GUTTER), r, len(f))


def test_a_chart_hundreds_of_faces_long_is_one_chart():
    from nero_amd import mesh as M
    v, f = A.mesh_of('tube')
    r = A.ref_charts('tube')
    assert r['K'] == 45 and r['n_faces'].max() > 500                 # the long sides of the tube
    chart, _, _, ci = M.face_charts_device(*_dev(v, f))
    assert _eq(chart, r['chart']) and _eq(ci.n_faces, r['n_faces'])


# ---- the smallest shapes ------------------------------------------------------------------------------------------------------------------
def _strip(T):
    """T triangles in a row, flat for the first half and climbing steeply after it (two classes), windings kept consistent"""
    n = T + 2
    i = np.arange(n)
    z = np.where(i < n // 2, 0.0, (i - n // 2) * 0.9)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), z], -1).astype(np.float32)
    t = np.arange(T)
    f = np.where((t % 2 == 0)[:, None], np.stack([t, t + 1, t + 2], -1), np.stack([t + 1, t, t + 2], -1)).astype(np.int32)
    return v, f


def _small_cases():
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1], [0.3, -0.2, -1], [1, 0, 2], [1, 1, 2]], np.float32)
    nan_v = quad.copy()
    nan_v[2, 1] = np.nan
    tie = np.array([[0, 0, 0], [1, -1, 0], [0, 0, 1], [1, 1, 0], [2, 0, 0.5]], np.float32)       # (b - a) x (c - a) = (-1, -1, 0) and (1, -1, 0)
    I = lambda *rows: np.array(rows, np.int32).reshape(-1, 3)
    cases = {
        'no_triangle': (quad, I()),
        'no_vertex_no_triangle': (np.zeros((0, 3), np.float32), I()),
        'no_vertex_one_triangle': (np.zeros((0, 3), np.float32), I([0, 1, 2])),
        'one_triangle': (quad, I([0, 1, 2])),
        'two_on_an_edge_same_class': (quad, I([0, 1, 2], [0, 2, 3])),
        'two_on_an_edge_other_class': (quad, I([0, 1, 2], [1, 6, 7], [1, 7, 2])),
        'three_on_one_edge': (quad, I([0, 1, 2], [0, 2, 3], [0, 2, 4], [0, 3, 4])),
        'a_face_listed_twice': (quad, I([0, 1, 2], [0, 2, 3], [0, 1, 2])),
        'a_face_listed_twice_alone': (quad, I([0, 1, 2], [0, 1, 2])),
        'a_b_a': (quad, I([0, 1, 2], [0, 2, 0], [0, 2, 3], [3, 3, 3])),
        'zero_area_distinct_indices': (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 1, 0]], np.float32), I([0, 1, 2], [0, 1, 3])),
        'index_out_of_range': (quad, I([0, 1, 2], [0, 2, 8], [0, 2, 3], [-1, 1, 2], [0, 2 ** 31 - 1, 3])),
        'nan_vertex': (nan_v, I([0, 1, 2], [0, 2, 3], [0, 3, 5], [0, 5, 1])),
        'class_tie': (tie, I([0, 1, 2], [0, 3, 2], [0, 1, 4])),
    }
    for T in (63, 64, 65, 255, 256, 257):
        cases[f'strip_{T}'] = _strip(T)
    return cases


SMALL = _small_cases()


@pytest.mark.parametrize('name', list(SMALL))
def test_the_smallest_shapes(name):
    v, f = SMALL[name]
    r = A.atlas(v, f, 64, GUTTER)
    if name == 'three_on_one_edge':
        assert r['nonmanifold'] == 1 and (r['nbr'][[0, 1, 2], [2, 0, 0]] == -1).all()    # no joins across the edge (0, 2)
        assert r['chart'][0] != r['chart'][1]                        # ... so the two flat faces are two charts
    if name == 'a_face_listed_twice':
        assert r['nonmanifold'] == 1 and r['K'] == 2 and r['chart'].tolist() == [0, 1, 0]     # joined across the edges the two copies share alone
    if name == 'class_tie':
        assert r['face_class'].tolist()[:2] == [1, 0]                # |n_x| == |n_y|: the lowest axis
    if name == 'two_on_an_edge_other_class':
        assert r['K'] == 2 and r['nbr'][0, 1] == 2 and r['chart'].tolist() == [0, 1, 1]
    if name in ('a_b_a', 'zero_area_distinct_indices', 'index_out_of_range', 'nan_vertex', 'no_vertex_one_triangle'):
        assert r['chartless'] > 0 and r['vt_vertex'][-1] == -1
    if name.startswith('strip_'):
        assert r['K'] == 2 and r['chartless'] == 0 and r['n_faces'].sum() == len(f)
    assert_api_equals(v, f, r, 64)
    assert_cabi_equals(cabi_atlas(v, f, 64, GUTTER), r, len(f))


def test_refused_sizes_and_null_pointers():
    from nero_amd import _lib as L
    from nero_amd import texture as TX
    lib = L.lib
    s = L.stream_ptr()
    one = torch.zeros(64, dtype=torch.int32, device='cuda')
    q = one.data_ptr()
    big_T, big_V = (2 ** 31) // 3 + 1, 2 ** 31
    assert lib.nero_mesh_face_adjacency_workspace_bytes(big_T) == 0 and lib.nero_mesh_chart_corners_workspace_bytes(big_T) == 0
    assert lib.nero_mesh_chart_label_workspace_bytes(big_T) == 0
    assert lib.nero_mesh_face_adjacency(q, big_T, 3, q, q, q, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_face_adjacency(q, 1, big_V, q, q, q, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_face_adjacency(q, -1, 3, q, q, q, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_chart_label(q, q, big_T, 3, q, q, q, q, q, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_chart_stats(q, q, big_T, 3, q, q, 1, q, q, q, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_chart_corners_count(q, big_T, 3, q, 1, q, q, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_chart_corners_emit(big_T, q, q, q, q, 1, s) == ERR_UNSUPPORTED
    assert lib.nero_mesh_face_adjacency(None, 1, 3, q, q, q, s) == ERR_ARG and lib.nero_mesh_face_adjacency(q, 1, 3, q, q, None, s) == ERR_ARG
    assert lib.nero_mesh_chart_label(q, q, 1, 3, q, q, None, q, q, s) == ERR_ARG and lib.nero_mesh_chart_label(q, q, 1, 3, q, q, q, q, None, s) == ERR_ARG
    assert lib.nero_mesh_chart_stats(q, q, 1, 3, q, q, 1, q, q, None, s) == ERR_ARG and lib.nero_mesh_chart_stats(q, q, 1, 3, q, q, 2, q, q, q, s) == ERR_ARG
    assert lib.nero_mesh_chart_corners_count(q, 1, 3, q, 1, None, q, s) == ERR_ARG and lib.nero_mesh_chart_corners_emit(1, None, q, q, q, 1, s) == ERR_ARG
    for size in (0, -1, 16385):
        assert lib.nero_mesh_chart_uv(q, 3, q, q, 1, q, q, q, 1, 1.0, size, q, s) == ERR_ARG
        assert lib.nero_uv_overlap_count(q, 3, q, 1, size, 8, q, q, s) == ERR_ARG and lib.nero_uv_overlap_count(q, 3, q, 1, 8, size, q, q, s) == ERR_ARG
        assert lib.nero_uv_overlap_count_workspace_bytes(1, size, 8) == 0
    assert lib.nero_mesh_chart_uv(q, 3, q, q, 1, q, q, q, 1, float('nan'), 8, q, s) == ERR_ARG
    assert lib.nero_mesh_chart_uv(q, 3, q, q, 1, q, q, q, 1, -1.0, 8, q, s) == ERR_ARG
    assert lib.nero_mesh_chart_uv(q, 3, q, q, 1, q, q, q, 1, 1.0, 8, None, s) == ERR_ARG
    assert lib.nero_uv_overlap_count(q, 3, q, 1, 8, 8, q, None, s) == ERR_ARG and lib.nero_uv_overlap_count(q, 3, None, 1, 8, 8, q, q, s) == ERR_ARG
    torch.cuda.synchronize()
    assert int(one.abs().sum()) == 0                                 # nothing was written
    with pytest.raises(ValueError):
        TX.chart_atlas(*_dev(*SMALL['one_triangle']), 0)
    with pytest.raises(ValueError):
        TX.chart_atlas(*_dev(*A.mesh_of('tube')), 20, 3)             # 45 charts of one texel need 27
    with pytest.raises(ValueError):
        TX.chart_atlas(*_dev(*A.mesh_of('tube')), 128, 4, texels_per_unit=50.0)


def test_a_capacity_that_is_too_small_writes_nothing():
    v, f = A.mesh_of((2, 9, 11))
    r = A.ref_atlas((2, 9, 11), 128, GUTTER)
    o = cabi_atlas(v, f, 128, GUTTER, vt_cap=len(r['vt']) - 1)
    assert o['n_vt'] == len(r['vt']) and o['emit_rc'] == ERR_ARG
    from nero_amd import _lib as L
    assert b'capacity' in L.lib.nero_last_error()
    for k in ('ft', 'vt_vertex', 'vt_chart'):
        assert o['guards'][k].untouched(), k
    o = cabi_atlas(v, f, 128, GUTTER, vt_cap=len(r['vt']) + 5)       # a larger capacity: the first n_vt entries, the rest untouched
    n = len(r['vt'])
    assert o['emit_rc'] == 0 and np.array_equal(o['vt_vertex'][:n], r['vt_vertex']) and (o['vt_vertex'][n:] == GUARD).all()
    assert np.array_equal(o['vt_chart'][:n], r['vt_chart']) and (o['vt_chart'][n:] == GUARD).all()


# ---- determinism and renumbering ----------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    from nero_amd import texture as TX
    vd, fd = _dev(*A.mesh_of((40, 33, 27)))
    a = TX.chart_atlas(vd, fd, 2048, GUTTER)
    b = TX.chart_atlas(vd, fd, 2048, GUTTER)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    for k in ('chart', 'face_class', 'nbr', 'vt_vertex', 'vt_chart'):
        assert torch.equal(getattr(a[2], k), getattr(b[2], k)), k
    assert a[2].scale == b[2].scale and np.array_equal(a[2].rects, b[2].rects) and a[2].overlap_texels == b[2].overlap_texels
    assert torch.equal(a[2].charts.box.view(torch.int32), b[2].charts.box.view(torch.int32)) and torch.equal(a[2].charts.n_faces, b[2].charts.n_faces)


def test_renumbering_the_faces_gives_the_same_partition():
    from nero_amd import mesh as M
    v, f = A.mesh_of((24, 20, 18))
    old = A.ref_charts((24, 20, 18))
    rg = np.random.default_rng(5)
    perm = rg.permutation(len(f))                                    # new face j is old face perm[j]
    f2 = np.stack([np.roll(t, k) for t, k in zip(f[perm], rg.integers(0, 3, len(f)))]).astype(np.int32)
    chart, cls, _, ci = M.face_charts_device(*_dev(v, f2))
    r2 = A.charts(v, f2)
    assert _eq(chart, r2['chart']) and _eq(cls, r2['face_class']) and ci.K == old['K'] and ci.n_chartless == old['chartless']
    now = chart.cpu().numpy()
    pairs = np.unique(np.stack([old['chart'][perm], now], 1), axis=0)                 # faces share a chart now exactly when they did before
    assert len(pairs) == old['K'] + 1 and len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs)
    assert np.array_equal(cls.cpu().numpy(), old['face_class'][perm])                 # a rotation of the corners keeps the class


# ---- overlap and coverage -----------------------------------------------------------------------------------------------------------------
def test_uv_overlap_equals_the_count_of_the_rule():
    from nero_amd import texture as TX
    r = A.ref_atlas('ramp', 64, GUTTER)
    _, cover = TR.raster(r['vt'], r['ft'], 64, 64, count=True)
    want = int((cover > 1).sum())
    assert want > 100 and TX.uv_overlap(r['vt'], r['ft'], 64, 64) == want
    _, cover = TR.raster(r['vt'], r['ft'], 131, 70, count=True)       # blocks of the walk cut by the map's edge, h != w
    assert TX.uv_overlap(r['vt'], r['ft'], 131, 70) == int((cover > 1).sum()) > 0
    for name, (vt, ft, h, w, _) in TR.special_cases().items():
        _, cover = TR.raster(vt, ft, h, w, count=True)
        assert TX.uv_overlap(vt, ft, h, w) == int((cover > 1).sum()), name
    assert TX.uv_overlap(*TR.special_cases()['overlap_lowest_wins'][:4]) > 0 and TX.uv_overlap(*TR.special_cases()['diagonal_through_centres'][:4]) == 0
    assert TX.uv_overlap(np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), 8, 8) == 0
    for h, w, nx, ny, seed in TR.GRID_CASES:                          # a triangulation of the square covers nothing twice
        assert TX.uv_overlap(*TR.jittered_grid(h, w, nx, ny, seed), h, w) == 0


@pytest.mark.parametrize('name', ['sphere', 'tube', (2, 9, 11), 'box'], ids=str)
def test_the_device_raster_keeps_charts_in_their_rectangles_and_a_gutter_apart(name):
    from nero_amd import texture as TX
    v, f = A.mesh_of(name)
    size = 128
    vt, ft, info = TX.chart_atlas(*_dev(v, f), size, GUTTER)
    chart = info.chart.cpu().numpy()
    assert info.overlap_texels == 0
    for factor in (1, 2):
        tri_id = TX.rasterize_uv(vt, ft, size * factor, size * factor).cpu().numpy()
        assert (tri_id >= 0).sum() > 0.1 * info.fill * (size * factor) ** 2
        A.assert_gutter_and_containment(A.chart_map(tri_id, chart), info.rects, GUTTER, factor)
        assert TX.uv_overlap(vt, ft, size * factor, size * factor) == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import build_material_case, golden_mesh, load_golden
    _, meta = load_golden('mat_bell')
    ref = build_material_case(meta)
    net = NeROMaterialRenderer({'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell'}, mesh=golden_mesh())
    net.load_state_dict(ref.state_dict())
    return net.cuda()


def test_bake_with_the_chart_atlas_end_to_end(net, tmp_path):
    from nero_amd import texture as TX
    tri = TX.bake_materials(net, size=128)
    cha = TX.bake_materials(net, size=128, atlas='charts')
    info = cha['atlas_info']
    assert 6 <= info.n_charts <= 40 and info.overlap_texels == 0 and info.charts.n_chartless == 0
    assert int(cha['mask'].sum()) > int(tri['mask'].sum())           # the charts use more of the map than one chart per triangle
    assert tuple(cha['albedo'].shape) == (128, 128, 3) and cha['albedo'].dtype == torch.uint8
    vt, ft = cha['vt'], cha['ft']
    assert torch.is_tensor(vt) and vt.is_cuda and ft.shape == (net.mesh_triangles.shape[0], 3)
    full = TX.rasterize_uv(vt, ft, 256, 256) >= 0                     # the bake's mask: a texel any of whose four supersamples is covered
    assert torch.equal(cha['mask'], full.view(128, 2, 128, 2).any(dim=3).any(dim=1))
    again = TX.bake_materials(net, vt=vt, ft=ft, size=128)           # the returned atlas is accepted as it is
    for k in ('albedo', 'metallic', 'roughness', 'mask'):
        assert torch.equal(again[k], cha[k]), k
    # the default is today's behaviour: an explicit simple_atlas, byte for byte
    svt, sft = TX.simple_atlas(net.mesh_vertices, net.mesh_triangles, 128)
    exp = TX.bake_materials(net, vt=svt, ft=sft, size=128)
    named = net.extract_texture_maps(size=128, atlas='triangles')
    for k in ('albedo', 'metallic', 'roughness', 'mask'):
        assert torch.equal(tri[k], exp[k]) and torch.equal(tri[k], named[k]), k
    assert np.array_equal(tri['vt'], svt) and np.array_equal(tri['ft'], sft) and 'atlas_info' not in tri
    with pytest.raises(ValueError):
        TX.bake_materials(net, size=128, atlas='lscm')
    # the OBJ round trip
    obj = TX.write_textured_obj(str(tmp_path), net.mesh_vertices, net.mesh_triangles, vt, ft, cha, name='mesh_7')
    back = TX.read_textured_obj(obj)
    assert np.array_equal(back['f'], net.mesh_triangles) and np.array_equal(back['ft'], ft.cpu().numpy())
    assert np.abs(back['vt'].astype(np.float64) - vt.cpu().numpy()).max() <= 2.0 ** -24          # u exact, v through 1 - (1 - v)
    assert np.array_equal(back['albedo'], cha['albedo'].cpu().numpy()) and np.array_equal(back['roughness'], cha['roughness'].cpu().numpy())
    assert np.array_equal(back['vt'][:, 0], vt.cpu().numpy()[:, 0])


def test_the_script_with_the_chart_atlas(tmp_path, capsys):
    from nero_amd.mesh import write_ply
    from tests.helpers import golden_mesh
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import extract_texture_maps as E
    finally:
        sys.path.pop(0)
    v, f = golden_mesh()
    ply, out = str(tmp_path / 'mesh.ply'), str(tmp_path / 'out')
    write_ply(ply, v, f)
    E.main(['--mesh', ply, '--atlas', 'charts', '--gutter', '3', '--size', '64', '--ssaa', '1', '--pad', '4', '--out', out, '--name', 'mesh_3'])
    cap = capsys.readouterr()
    rep = json.loads(cap.out.strip().split('\n')[-1])
    assert rep['atlas'] == 'chart_atlas' and rep['charts'] >= 6 and rep['overlap_texels'] == 0 and 0 < rep['fill'] < 1 and rep['scale'] > 0
    assert 'charts' in cap.err and 'warning' not in cap.err
    for name in ('mesh_3.obj', 'mesh_3.mtl', 'feat0_3.png', 'feat1_3.png', 'feat2_3.png', 'mesh_3_atlas.npz'):
        assert os.path.exists(os.path.join(out, name)), name
    z = np.load(os.path.join(out, 'mesh_3_atlas.npz'))
    r = A.atlas(v, f, 64, 3)
    assert np.array_equal(z['ft'], r['ft']) and np.array_equal(z['vt'].view(np.int32), r['vt'].view(np.int32))
    assert np.array_equal(z['vt_vertex'], r['vt_vertex']) and np.array_equal(z['rects'], r['rects']) and float(z['scale']) == r['scale']
