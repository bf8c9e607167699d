"""GPU tier: the mesh simplification (nero_amd/csrc/mesh_simplify.hip through nero_amd.mesh and through the C ABI) against the numpy
restatement tests/mesh_simplify_ref.py (pinned by tests/test_mesh_simplify_cpu.py).  Everything integer is exact: V', T', the cell keys,
the triangles, vmap, fmap and the counts.  The float64 positions carry bounds with their origin:
  'mean'     (m_v + 2) 2^-53 |cbar|_inf per axis, m_v the vertices of the cell: the two sums may differ by their order, the quotient rounds;
  'quadric'  8 * 3001 * (m + 16) 2^-53 max(|x_unclamped - cbar|_inf, cell), m the contributions of the cell: the condition bound of the
             regularised system, the length of the sums, the scale of the solution.  A case counts only where the restatement's own error
             (its np.longdouble evaluation) is below a quarter of the bound.
The worst ratio of error to bound is printed by test_agreement_with_the_restatement."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mcubes_ref as R
from tests import mesh_clean_ref as MR
from tests import mesh_simplify_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ['sphere', 'torus', 'two_spheres', 'tube', 'box'] + sorted(MR.RANDOM_SHAPES)
U = 2.0 ** -53
GUARD, ISENT, FSENT = 7, -77, -12345.0


def mesh_of(name):
    return S.box_mesh() if name == 'box' else MR.mesh_of(name)


def _dev(v, f):
    return (torch.from_numpy(np.array(v, np.float32)).cuda().reshape(-1, 3),
            torch.from_numpy(np.array(f, np.int32)).cuda().reshape(-1, 3))


def _eq(t, a):
    a = np.ascontiguousarray(a)
    return tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


@functools.lru_cache(maxsize=None)
def _ref(name, cell, placement, dedup=True):
    o = S.simplify(*mesh_of(name), cell, placement=placement, dedup=dedup, with_longdouble=True)
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def _position_ratio(pos, ref, placement):
    """-> the largest error / bound over the output vertices (0 for an empty mesh); asserts that the restatement's own error is below a
    quarter of the bound everywhere, so that every vertex counts"""
    x = ref['verts']
    if len(x) == 0:
        return 0.0
    if placement == 'mean':
        bound = ((ref['m_v'] + 2) * U * np.abs(ref['cbar']).max(axis=1))[:, None]
    else:
        scale = np.maximum(np.abs(ref['x_unclamped'] - ref['cbar']).max(axis=1), ref['cell'])
        bound = (8 * 3001 * (ref['m'] + 16) * U * scale)[:, None]
    err = np.abs(pos - x)
    if 'verts_ld' in ref and np.finfo(np.longdouble).eps < 1e-18:
        own = np.abs(ref['verts_ld'] - x).astype(np.float64)
        assert (own <= 0.25 * bound).all()
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    return float((err[bound[:, 0] > 0] / bound[bound[:, 0] > 0]).max()) if (bound > 0).any() else 0.0


def _assert_result(v2, f2, info, ref, placement):
    """the Python API's result against the restatement -> the position ratio"""
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32 and info.cell_key.dtype == torch.int64
    assert info.positions64.dtype == torch.float64 and info.vmap.dtype == torch.int32 and info.fmap.dtype == torch.int32
    assert v2.shape == (len(ref['verts']), 3) and f2.shape == (len(ref['tris']), 3)
    assert _eq(info.cell_key, ref['cell_key']) and _eq(f2, ref['tris']) and _eq(info.vmap, ref['vmap']) and _eq(info.fmap, ref['fmap'])
    assert info.n_survivors == ref['n_survivors'] and info.n_duplicates == ref['n_duplicates']
    assert info.cell == ref['cell'] and list(info.origin) == ref['origin'].tolist()
    assert torch.equal(v2.view(torch.int32), info.positions64.float().view(torch.int32))       # the float32 rounding, bit for bit
    return _position_ratio(info.positions64.cpu().numpy(), ref, placement)


_worst = {'mean': 0.0, 'quadric': 0.0}


@pytest.mark.parametrize('dedup', [True, False], ids=['dedup', 'all'])
@pytest.mark.parametrize('placement', ['quadric', 'mean'])
@pytest.mark.parametrize('cell', [1.0, 2.0, 3.0])
@pytest.mark.parametrize('name', FIXTURES, ids=str)
def test_agreement_with_the_restatement(name, cell, placement, dedup):
    from nero_amd.mesh import simplify_mesh_device
    ref = _ref(name, cell, placement, dedup)
    v2, f2, info = simplify_mesh_device(*_dev(*mesh_of(name)), cell=cell, placement=placement, dedup=dedup)
    assert info.k is None
    ratio = _assert_result(v2, f2, info, ref, placement)
    _worst[placement] = max(_worst[placement], ratio)
    print(f'{name} cell {cell} {placement}: V {len(mesh_of(name)[0])} -> {len(v2)}, T {len(mesh_of(name)[1])} -> {len(f2)}, duplicates '
          f'{info.n_duplicates}, error / bound {ratio:.3e} (worst so far: mean {_worst["mean"]:.3e}, quadric {_worst["quadric"]:.3e})')
    if name == (24, 20, 18) and cell == 2.0 and dedup:
        assert info.n_duplicates == 565                               # the de-duplication has something to do


# ---- the C ABI with guard words round every output ---------------------------------------------------------------------------------------
def _guarded(rows, width, dtype):
    sent = ISENT if dtype in (torch.int32, torch.int64) else FSENT
    buf = torch.full((rows + 2 * GUARD, width), sent, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + rows]


def _untouched(buf, rows):
    sent = ISENT if buf.dtype in (torch.int32, torch.int64) else FSENT
    return bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + rows:] == sent).all())


def _raw(v, f, cell, origin=None, placement='quadric', dedup=True):
    """nero_mesh_simplify_count / _emit called directly; every output lies between guard rows that must stay untouched, and the rows of the
    triangle buffer behind T' too.  -> dict like the restatement's"""
    from nero_amd import _lib as L
    vd, fd = _dev(v, f)
    V, T = vd.shape[0], fd.shape[0]
    o = (C.c_double * 3)(*(S.default_origin(v) if origin is None else origin))
    need = int(L.lib.nero_mesh_simplify_workspace_bytes(V, T))
    assert need > 0
    wsb = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device='cuda')     # (256 guard bytes on either side keep the alignment)
    ws = wsb[256:256 + need]
    tb, totals = _guarded(1, 4, torch.int32)
    p = lambda t: t.data_ptr() if t.numel() else None
    s = L.stream_ptr()
    for faces_only in (1, 0):
        L.check(L.lib.nero_mesh_simplify_count(p(vd), p(fd), T, V, cell, o, faces_only, p(ws), p(totals), s))
        tot = totals[0].tolist()
        if faces_only:
            assert tot[0] == -1
            n_first = tot[1]
    V2, n, bad_v, bad_t = tot
    assert n == n_first and bad_v == 0 and bad_t == 0 and _untouched(tb, 1)
    posb, pos = _guarded(V2, 3, torch.float64)
    v2b, v2 = _guarded(V2, 3, torch.float32)
    keyb, key = _guarded(V2, 1, torch.int64)
    f2b, f2 = _guarded(n, 3, torch.int32)
    vmb, vmap = _guarded(V, 1, torch.int32)
    fmb, fmap = _guarded(T, 1, torch.int32)
    nb, n_out = _guarded(1, 1, torch.int64)
    L.check(L.lib.nero_mesh_simplify_emit(p(vd), p(fd), T, V, cell, o, {'mean': 0, 'quadric': 1}[placement], int(dedup), p(ws), p(pos), p(v2),
                                          p(key), V2, p(f2), n, p(vmap), p(fmap), p(n_out), s))
    torch.cuda.synchronize()
    T2 = int(n_out[0, 0])
    assert 0 <= T2 <= n
    for buf, rows in ((posb, V2), (v2b, V2), (keyb, V2), (f2b, T2), (vmb, V), (fmb, T), (nb, 1), (tb, 1)):
        assert _untouched(buf, rows)
    assert bool((wsb[:256] == 0x5A).all()) and bool((wsb[256 + need:] == 0x5A).all())
    return {'verts': pos.cpu().numpy(), 'verts32': v2.cpu().numpy(), 'cell_key': key[:, 0].cpu().numpy(), 'tris': f2[:T2].cpu().numpy(),
            'vmap': vmap[:, 0].cpu().numpy(), 'fmap': fmap[:, 0].cpu().numpy(), 'n_survivors': n, 'n_duplicates': n - T2}


def _assert_raw(got, ref, placement):
    for k in ('cell_key', 'tris', 'vmap', 'fmap'):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert got['n_survivors'] == ref['n_survivors'] and got['n_duplicates'] == ref['n_duplicates']
    assert np.array_equal(got['verts32'].view(np.int32), got['verts'].astype(np.float32).view(np.int32))
    return _position_ratio(got['verts'], ref, placement)


@pytest.mark.parametrize('dedup', [True, False], ids=['dedup', 'all'])
@pytest.mark.parametrize('placement', ['quadric', 'mean'])
@pytest.mark.parametrize('name,cell', [('sphere', 2.0), ((24, 20, 18), 2.0), ((2, 9, 11), 1.0)], ids=str)
def test_no_write_outside_the_outputs(name, cell, placement, dedup):
    v, f = mesh_of(name)
    _assert_raw(_raw(v, f, cell, placement=placement, dedup=dedup), _ref(name, cell, placement, dedup), placement)


# ---- edge shapes ------------------------------------------------------------------------------------------------------------------------
def test_empty_meshes():
    from nero_amd.mesh import simplify_mesh_device
    ev, ef = torch.zeros((0, 3), device='cuda'), torch.zeros((0, 3), dtype=torch.int32, device='cuda')
    pv = torch.arange(15, dtype=torch.float32, device='cuda').reshape(5, 3)
    for v, f in ((ev, ef), (pv, ef)):
        for kw in ({'cell': 1.0}, {'target_faces': 10}, {'cell': 2.0, 'placement': 'mean', 'dedup': False}):
            v2, f2, info = simplify_mesh_device(v, f, **kw)
            assert v2.shape == (0, 3) and v2.dtype == torch.float32 and f2.shape == (0, 3) and f2.dtype == torch.int32
            assert info.cell_key.shape == (0,) and info.positions64.shape == (0, 3) and info.fmap.shape == (0,)
            assert info.vmap.tolist() == [-1] * len(v) and info.n_survivors == 0 and info.n_duplicates == 0
    # the kernels themselves on V = 5, T = 0 and on V = 0
    for v in (pv.cpu().numpy(), np.zeros((0, 3), np.float32)):
        got = _raw(v, np.zeros((0, 3), np.int32), 1.0, origin=(0.0, 0.0, 0.0))
        assert got['verts'].shape == (0, 3) and got['tris'].shape == (0, 3) and got['vmap'].tolist() == [-1] * len(v)


def test_single_triangles():
    v = np.array([[0.25, 0.5, 0.5], [1.5, 0.5, 0.25], [0.5, 1.75, 0.5]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    for placement in ('quadric', 'mean'):
        ref = S.simplify(v, f, 1.0, origin=(0, 0, 0), placement=placement, with_longdouble=True)
        assert ref['tris'].tolist() == [[0, 2, 1]] and ref['cell_key'].tolist() == [0, 1 << 21, 1 << 42]
        _assert_raw(_raw(v, f, 1.0, origin=(0, 0, 0), placement=placement), ref, placement)
        # the same triangle inside one cell: nothing survives, no cell is used
        got = _raw(v, f, 2.0, origin=(0, 0, 0), placement=placement)
        assert got['verts'].shape == (0, 3) and got['tris'].shape == (0, 3) and got['vmap'].tolist() == [-1] * 3 and got['fmap'].tolist() == [-1]
        assert got['n_survivors'] == 0


@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257])
def test_partial_waves_and_workgroups(n):
    """the first n faces of the sphere over all its vertices: T at the edges of a wave and of a workgroup, and nearly every vertex
    unreferenced -- such vertices enter the means and never become output on their own"""
    v, f = mesh_of('sphere')
    for placement in ('quadric', 'mean'):
        ref = S.simplify(v, f[:n], 2.0, placement=placement, with_longdouble=True)
        assert 0 < len(ref['verts']) < 300 and (ref['m_v'].sum() > len(np.unique(f[:n])))      # unreferenced vertices in the used cells
        assert (ref['vmap'] < 0).sum() > 7000
        _assert_raw(_raw(v, f[:n], 2.0, placement=placement), ref, placement)


def test_unreferenced_vertices_enter_the_mean_only():
    from nero_amd.mesh import simplify_mesh_device
    v = np.array([[0, 0, 0], [2.5, 0, 0], [0, 2.5, 0], [0.5, 0.5, 0.5], [7, 7, 7]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    v2, f2, info = simplify_mesh_device(*_dev(v, f), cell=1.0, origin=(0, 0, 0), placement='mean')
    assert info.vmap.tolist() == [0, 2, 1, 0, -1] and f2.tolist() == [[0, 2, 1]]
    assert info.positions64.tolist() == [[0.25, 0.25, 0.25], [0.0, 2.5, 0.0], [2.5, 0.0, 0.0]]


@pytest.mark.parametrize('name', ['sphere', (40, 33, 27)], ids=str)
def test_a_handful_of_cells_with_thousands_of_contributions(name):
    """cell = the longest side D of the box: at most 8 cells -- on these meshes no triangle reaches three of them, and the result is empty;
    D / 2: 9 and 12 cells that sum thousands of contributions each, over several pieces: the second level of the fixed-order sum"""
    from nero_amd.mesh import simplify_mesh_device
    v, f = mesh_of(name)
    D = S.longest_side(v)
    for placement in ('quadric', 'mean'):
        ref = S.simplify(v, f, D, placement=placement, with_longdouble=True)
        v2, f2, info = simplify_mesh_device(*_dev(v, f), cell=D, placement=placement)
        assert len(ref['verts']) <= 8
        _assert_result(v2, f2, info, ref, placement)
        ref = S.simplify(v, f, D / 2, placement=placement, with_longdouble=True)
        assert 8 <= len(ref['verts']) <= 27 and ref['m'].max() > 2 * 2048 and (name == 'sphere' or ref['m_v'].max() > 2 * 2048)
        ratio = _assert_result(*simplify_mesh_device(*_dev(v, f), cell=D / 2, placement=placement), ref, placement)
        print(f'{name} cell D / 2 {placement}: {len(ref["verts"])} cells, up to {ref["m"].max()} contributions, error / bound {ratio:.3e}')


def test_an_origin_below_the_box():
    from nero_amd.mesh import simplify_mesh_device
    v, f = mesh_of('torus')
    origin = (-3.25, -0.7, -11.0)
    ref = S.simplify(v, f, 2.0, origin=origin, with_longdouble=True)
    assert not np.array_equal(ref['cell_key'], _ref('torus', 2.0, 'quadric')['cell_key'])
    _assert_result(*simplify_mesh_device(*_dev(v, f), cell=2.0, origin=origin), ref, 'quadric')
    with pytest.raises(ValueError, match='vertices'):                 # an origin above the smallest vertex: negative cell indices
        simplify_mesh_device(*_dev(v, f), cell=2.0, origin=(20.0, 0.0, 0.0))


def test_a_vertex_on_a_cell_boundary_belongs_to_the_upper_cell():
    from nero_amd.mesh import simplify_mesh_device
    cell, origin = 0.75, (0.5, 0.5, 0.5)
    below = np.nextafter(np.float32(2.75), np.float32(0))
    v = np.array([[2.75, 0.6, 0.6], [below, 1.4, 0.6], [0.6, 0.6, 2.0], [0.5, 0.5, 0.5]], np.float32)   # 2.75 = 0.5 + 3 * 0.75 exactly
    f = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    assert np.floor((np.float64(v[0, 0]) - 0.5) / 0.75) == 3.0 and np.floor((np.float64(below) - 0.5) / 0.75) == 2.0
    ref = S.simplify(v, f, cell, origin=origin)
    assert ref['cell_key'].tolist() == [0, 2, (2 << 42) | (1 << 21), 3 << 42]
    v2, f2, info = simplify_mesh_device(*_dev(v, f), cell=cell, origin=origin)
    assert info.cell_key.tolist() == ref['cell_key'].tolist() and info.vmap.tolist() == [3, 2, 1, 0] and f2.tolist() == [[3, 2, 1], [1, 2, 0]]
    # a division, not a multiplication by the reciprocal: (x - o) / cell and (x - o) * (1 / cell) fall on different sides of an integer
    xs = np.arange(1, 4000, dtype=np.float32) * np.float32(0.25)
    differ = np.nonzero(np.floor(xs.astype(np.float64) / 1.1) != np.floor(xs.astype(np.float64) * (1.0 / 1.1)))[0]
    assert len(differ) > 50 and xs[differ[0]] == 16.5                # such points exist on this ladder (16.5 = 15 * 1.1, ...) ...
    w = np.zeros((len(xs) + 2, 3), np.float32)
    w[:len(xs), 0] = xs
    w[len(xs)] = (0, 5, 0)
    w[len(xs) + 1] = (0, 0, 5)
    g = np.stack([np.arange(len(xs)), np.full(len(xs), len(xs)), np.full(len(xs), len(xs) + 1)], 1).astype(np.int32)
    ref = S.simplify(w, g, 1.1, origin=(0, 0, 0), placement='mean')
    v2, f2, info = simplify_mesh_device(*_dev(w, g), cell=1.1, origin=(0, 0, 0), placement='mean')
    assert _eq(info.cell_key, ref['cell_key']) and _eq(info.vmap, ref['vmap']) and _eq(f2, ref['tris'])   # ... and land where numpy puts them


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_refused_input_raises_and_nothing_faults():
    from nero_amd.mesh import simplify_mesh_device
    v, f = mesh_of((2, 9, 11))
    for bad in (len(v), -1, 2 ** 31 - 1):
        g = f.copy()
        g[len(g) // 2, 1] = bad
        with pytest.raises(ValueError, match=f'1 of {len(f)} triangles'):
            simplify_mesh_device(*_dev(v, g), cell=1.0)
        with pytest.raises(ValueError, match='triangles'):
            simplify_mesh_device(*_dev(v, g), target_faces=100)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[7, 1] = bad
        with pytest.raises(ValueError, match='vertices'):
            simplify_mesh_device(*_dev(w, f), cell=1.0)
        with pytest.raises(ValueError, match=f'1 of {len(v)} vertices'):
            simplify_mesh_device(*_dev(w, f), cell=1.0, origin=S.default_origin(v))
        with pytest.raises(ValueError, match='vertices'):
            simplify_mesh_device(*_dev(w, f), target_faces=100)
    with pytest.raises(ValueError, match='vertices'):                 # 10 / 2^21 = 4.8e-6: an index past 2^21
        simplify_mesh_device(*_dev(v, f), cell=1e-6)
    vd, fd = _dev(v, f)
    for kw in ({}, {'cell': 1.0, 'target_faces': 5}, {'cell': 0.0}, {'cell': -1.0}, {'cell': float('nan')}, {'cell': float('inf')},
               {'cell': 1.0, 'placement': 'median'}, {'target_faces': -1}, {'target_faces': 2.5}, {'cell': 1.0, 'origin': (0.0, float('nan'), 0.0)}):
        with pytest.raises(ValueError):
            simplify_mesh_device(vd, fd, **kw)
    for args in ((vd.cpu(), fd), (vd, fd.long()), (vd.double(), fd), (vd[:, :2], fd), (vd, None)):
        with pytest.raises(TypeError):
            simplify_mesh_device(*args, cell=1.0)
    torch.cuda.synchronize()
    _assert_result(*simplify_mesh_device(vd, fd, cell=1.0), _ref((2, 9, 11), 1.0, 'quadric'), 'quadric')    # the device is as it was


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
def _bits(v2, f2, info):
    return [v2.view(torch.int32), f2, info.cell_key, info.positions64.view(torch.int64), info.vmap, info.fmap]


def test_two_runs_are_bit_identical():
    from nero_amd.mesh import simplify_mesh_device
    vd, fd = _dev(*mesh_of((40, 33, 27)))
    for kw in ({'cell': 2.0}, {'cell': 1.0, 'placement': 'mean', 'dedup': False}, {'target_faces': 10000}):
        a, b = simplify_mesh_device(vd, fd, **kw), simplify_mesh_device(vd, fd, **kw)
        assert len(a[1]) > 1000 and all(torch.equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))
        assert (a[2].n_survivors, a[2].n_duplicates, a[2].k, a[2].cell) == (b[2].n_survivors, b[2].n_duplicates, b[2].k, b[2].cell)


def test_result_does_not_depend_on_the_numbering():
    from nero_amd.mesh import simplify_mesh_device
    name = (40, 33, 27)
    v, f = mesh_of(name)
    rg = np.random.default_rng(5)
    new_of_old = rg.permutation(len(v))
    v2 = np.empty_like(v)
    v2[new_of_old] = v
    f2 = new_of_old[f][rg.permutation(len(f))].astype(np.int32)
    ref = _ref(name, 2.0, 'quadric')
    w, g, info = simplify_mesh_device(*_dev(v2, f2), cell=2.0)
    assert _eq(info.cell_key, ref['cell_key'])                         # the same cells ...
    key = ref['cell_key']
    triples = lambda t: np.unique(np.sort(key[t], axis=1), axis=0)     # (dedup keeps the first of each vertex set: which winding stays
    assert np.array_equal(triples(g.cpu().numpy()), triples(ref['tris']))    # depends on the order, the set does not)
    assert len(g) == len(ref['tris'])
    _position_ratio(info.positions64.cpu().numpy(), ref, 'quadric')    # ... and the same positions within the bound


# ---- the face budget --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,N', [('sphere', 1500), ((40, 33, 27), 10000)], ids=str)
def test_target_faces(name, N):
    from nero_amd.mesh import simplify_cells, simplify_mesh_device
    v, f = mesh_of(name)
    counts = S.counts_by_k(v, f)
    k = S.choose_k_bisect(lambda q: counts[q], N)
    assert k == S.choose_k_scan(counts, N)
    vd, fd = _dev(v, f)
    a = simplify_mesh_device(vd, fd, target_faces=N)
    D = S.longest_side(v)
    assert a[2].k == k and a[2].cell == simplify_cells(D, k) == S.simplify_cells(D, k) and len(a[1]) <= N
    assert a[2].n_survivors == counts[k] <= N
    b = simplify_mesh_device(vd, fd, cell=simplify_cells(D, k))
    assert b[2].k is None and all(torch.equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))
    _assert_result(*a, S.simplify(v, f, S.simplify_cells(D, k), with_longdouble=True), 'quadric')
    with pytest.raises(ValueError, match='target_faces'):
        simplify_mesh_device(vd, fd, target_faces=counts[0] - 1 if counts[0] else -1)
    if name == 'sphere':
        assert counts[0] == 0 and counts[1] == 12
        o = S.default_origin(v) - D / 2                               # n(0) > N: an origin that splits the coarsest cell
        assert S.survivor_count(v, f, D, origin=o) == 12
        with pytest.raises(ValueError, match='below the 12 faces'):
            simplify_mesh_device(vd, fd, target_faces=3, origin=o.tolist())


# ---- quality ----------------------------------------------------------------------------------------------------------------------------
def test_quadric_placement_finds_the_edges_of_the_box():
    from nero_amd.mesh import simplify_mesh_device
    vd, fd = _dev(*S.box_mesh())
    for cell in (2.0, 3.0, 4.0):
        mean = S.box_surface_distance(simplify_mesh_device(vd, fd, cell=cell, placement='mean')[2].positions64.cpu().numpy())
        quad = S.box_surface_distance(simplify_mesh_device(vd, fd, cell=cell, placement='quadric')[2].positions64.cpu().numpy())
        print(f'box, cell {cell}: mean distance to the surface, mean placement {mean:.4f}, quadric {quad:.4f}, ratio {quad / mean:.3f}')
        assert quad / mean <= 0.5


# ---- hand-offs --------------------------------------------------------------------------------------------------------------------------
def test_clean_up_then_simplification():
    from nero_amd.mesh import clean_mesh_device, simplify_mesh, simplify_mesh_device
    v, f = mesh_of('two_spheres')
    vc, fc, _ = clean_mesh_device(*_dev(v, f), keep='largest')
    vr, fr, _ = MR.clean(v, f, keep='largest')
    ref = S.simplify(vr, fr, 2.0, with_longdouble=True)
    v2, f2, info = simplify_mesh_device(vc, fc, cell=2.0)
    _assert_result(v2, f2, info, ref, 'quadric')
    assert R.euler_characteristic(ref['verts'], ref['tris']) == 2 and len(f2) < len(fr) // 3
    vn, fn, info_n = simplify_mesh(vr.astype(np.float64), fr.astype(np.int64), cell=2.0)       # the numpy entry point
    assert vn.dtype == np.float64 and fn.dtype == np.int64 and np.array_equal(fn, ref['tris'])
    assert np.array_equal(vn, info.positions64.cpu().numpy())


def test_extract_geometry_with_and_without_simplification():
    from bench import BELL, VARIANCE
    from nero_amd import mesh as M
    from nero_amd.renderer import NeROShapeRenderer
    from nero_amd.synthetic import perturb_state
    torch.manual_seed(6033)
    net = NeROShapeRenderer(dict(BELL), training=False)
    perturb_state(net, VARIANCE)
    net = net.cuda()
    lo, hi = (-1., -1., -1.), (1., 1., 1.)
    vd, fd = M.marching_cubes_device(net._sdf_grid(lo, hi, 48, 2 ** 21, 1.0), 0.0)
    assert len(fd) > 100
    v0, f0 = M.index_to_world(vd.cpu().numpy(), 48, lo, hi), fd.cpu().numpy().astype(np.int64)
    for kw in ({}, {'simplify': None}, {'clean': None, 'simplify': None}):
        v, f = net.extract_geometry(resolution=48, **kw)
        assert v.dtype == np.float64 and f.dtype == np.int64 and v.tobytes() == v0.tobytes() and f.tobytes() == f0.tobytes()
    vc, fc, _ = M.clean_mesh_device(vd, fd, keep='largest')
    vs, fs, info = M.simplify_mesh_device(vc, fc, cell=2.0)
    v, f = net.extract_geometry(resolution=48, clean={'keep': 'largest'}, simplify={'cell': 2.0})
    assert 0 < len(fs) < len(fc) and f.dtype == np.int64 and v.dtype == np.float64
    assert np.array_equal(f, fs.cpu().numpy().astype(np.int64)) and np.array_equal(v, M.index_to_world(vs.cpu().numpy(), 48, lo, hi))
    _assert_result(vs, fs, info, S.simplify(vc.cpu().numpy(), fc.cpu().numpy(), 2.0, with_longdouble=True), 'quadric')


def test_simplified_sphere_reaches_the_ray_tracer():
    from nero_amd.mesh import simplify_mesh_device
    from nero_amd.raytracing import RayTracer
    cell, scale = 2.0, 36.0                                            # (the tracer reports no hit beyond a distance of 10)
    v2, f2, _ = simplify_mesh_device(*_dev(*mesh_of('sphere')), cell=cell)
    assert len(f2) == 2860
    tracer = RayTracer((v2 / scale).contiguous(), f2)
    rg = np.random.default_rng(12)
    d = rg.normal(size=(2048, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = np.array([27.3, 27.6, 27.8])
    o = (centre + 30.0 * d) / scale
    _, _, t = tracer.trace(torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy((-d).astype(np.float32)).cuda())
    t = t.reshape(-1).double().cpu().numpy()
    assert (t < 10).all()                                              # the simplified surface is still closed: every ray hits
    assert np.abs(t * scale - 10.0).max() <= np.sqrt(3.0) * cell       # the analytic depth is 30 - 20


def test_script_simplifies_a_ply_to_a_face_budget(tmp_path):
    from nero_amd.mesh import read_ply, simplify_mesh_device, write_ply
    v, f = mesh_of('sphere')
    src, dst = str(tmp_path / 'sphere.ply'), str(tmp_path / 'out.ply')
    write_ply(src, v, f)
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'extract_mesh.py'), '--in', src, '--target-faces', '1500', '--out', dst],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    v2, f2 = read_ply(dst)
    assert 0 < len(f2) <= 1500 and f2.max() == len(v2) - 1
    va, fa, info = simplify_mesh_device(*_dev(v, f), target_faces=1500)
    assert np.array_equal(f2, fa.cpu().numpy()) and np.array_equal(v2.astype(np.float32), va.cpu().numpy())
    s = out['simplify']
    assert s['target_faces'] == 1500 and s['k'] == info.k and s['cell'] == info.cell and s['before'] == {'n_verts': len(v), 'n_faces': len(f)}
    assert s['after'] == {'n_verts': len(v2), 'n_faces': len(f2)} and s['n_duplicates'] == info.n_duplicates
