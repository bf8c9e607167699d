"""GPU tier: the surface sampler (nero_amd/csrc/surface_sample.hip through nero_amd.surface and through the C ABI) against the numpy
restatement tests/surface_ref.py (pinned by tests/test_surface_sample_cpu.py), BIT FOR BIT: the integer weights and their running sum, the
record {total, zero weights, e, B}, and for the samples the face, the barycentric weights, the point and the normal.  No tolerance is used
for any of them: the contract rounds every float64 operation on its own and the kernels are built without contraction.  The one bound in
here (the mix of a point from its REPORTED fp32 barycentric weights) carries its derivation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import surface_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FSENT, ISENT = 5, -12345.0, -77
OUTS = ('pts', 'face', 'bary', 'normal')


@pytest.fixture(scope='module')
def SF():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import surface
    return surface


def _tiled(T):
    """the first T triangles of copies of the squashed icosphere, copy k scaled by 0.5 + (k mod 7) / 7 and moved along x"""
    v, f = SR.squashed_icosphere()
    k = -(-T // len(f))
    s = (0.5 + (np.arange(k) % 7) / 7.0).astype(np.float32)
    vv = v[None] * s[:, None, None] + np.stack([np.arange(k, dtype=np.float32) * 0.01, np.zeros(k, np.float32), np.zeros(k, np.float32)], -1)[:, None]
    ff = f[None].astype(np.int64) + (np.arange(k, dtype=np.int64) * len(v))[:, None, None]
    return vv.reshape(-1, 3).astype(np.float32), ff.reshape(-1, 3)[:T].astype(np.int32)


def _one_and_a_half():
    """two triangles of doubled area 1.5 (the largest: 1.5 times a power of two, so e sits on no boundary) and a small one"""
    v = np.asarray([[0, 0, 0], [1.5, 0, 0], [1.5, 1, 0], [0, 1, 0], [0, 0, 1], [0.25, 0, 1], [0, 0.25, 1]], np.float32)
    return v, np.asarray([[0, 1, 2], [4, 5, 6], [0, 2, 3]], np.int32)


def _mesh(name):
    if name == 'icosphere':
        return SR.squashed_icosphere()
    if name in ('T1', 'T65'):
        v, f = SR.squashed_icosphere()
        return v, f[:int(name[1:])]
    if name == 'tiled':
        return _tiled(2 ** 20 + 3)
    if name == 'one_and_a_half':
        return _one_and_a_half()
    return SR.degenerate_mesh()[:2]


def _raw(SF, v, f, rec, first, n, n_total, seed, stratified, want=OUTS[1:]):
    """nero_surface_sample itself, every output between guard elements that must come back untouched -> {name: numpy}"""
    from nero_amd import _lib as L
    dev = torch.device('cuda', 0)
    vt, ft = torch.from_numpy(v).to(dev).contiguous(), torch.from_numpy(f).to(dev).contiguous()
    width = {'pts': 3, 'face': 1, 'bary': 2, 'normal': 3}
    buf = {k: torch.full(((n + 2 * GUARD) * width[k],), ISENT if k == 'face' else FSENT, dtype=torch.int32 if k == 'face' else torch.float32,
                         device=dev) for k in ('pts',) + tuple(want)}
    at = lambda k: buf[k][GUARD * width[k]:] if k in buf else None
    L.check(L.lib.nero_surface_sample(L.ptr(vt), len(v), L.ptr(ft), len(f), L.ptr(rec['cdf']), L.ptr(rec['info']), first, n, n_total, seed,
                                      int(stratified), L.ptr(at('pts')), L.ptr(at('face')), L.ptr(at('bary')), L.ptr(at('normal')), L.stream_ptr()))
    out = {}
    for k, b in buf.items():
        a, g = b.cpu().numpy(), GUARD * width[k]
        assert np.all(a[:g] == a[0]) and np.all(a[len(a) - g:] == a[0]) and a[0] in (ISENT, FSENT), k      # nothing written outside [0, n)
        out[k] = a[g:len(a) - g].reshape((n,) if k == 'face' else (n, width[k]))
    return out


def _same(got, ref, keys):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), (k, int((got[k] != ref[k]).sum()))     # the bits, -0 and all


@pytest.mark.parametrize('name', ['icosphere', 'T1', 'T65', 'tiled', 'one_and_a_half', 'degenerate'])
def test_cdf_equals_the_restatement_bit_for_bit(SF, name):
    v, f = _mesh(name)
    ref = SR.surface_cdf(v, f)
    rec = SF.surface_cdf(v, f)
    assert rec['cdf'].dtype == torch.int64 and rec['cdf'].is_cuda and tuple(rec['cdf'].shape) == (len(f),)
    cdf = rec['cdf'].cpu().numpy().astype(np.uint64)
    assert (rec['total'], rec['zero_weight'], rec['e'], rec['B']) == (ref['total'], ref['zero_weight'], ref['e'], ref['B'])
    assert np.array_equal(np.diff(cdf, prepend=np.uint64(0)), ref['w'])                # the weights
    assert np.array_equal(cdf, ref['cdf'])
    assert rec['info'].cpu().tolist() == [ref['total'], ref['zero_weight'], ref['e'], ref['B']] and rec['area'] == ref['area']
    if name == 'tiled':
        assert len(f) == 2 ** 20 + 3 and rec['B'] == 40                                 # L = 21 <= 22: the full 40 bits
    if name == 'one_and_a_half':
        assert float(ref['a2'].max()) == 1.5 and rec['e'] == 1
    if name == 'degenerate':
        assert rec['zero_weight'] == 6 and rec['total'] == 2 ** 40
    again = SF.surface_cdf(v, f)
    assert torch.equal(again['cdf'], rec['cdf']) and torch.equal(again['info'], rec['info'])


@pytest.mark.parametrize('stratified', [True, False])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 4097])
def test_samples_equal_the_restatement_bit_for_bit(SF, n, stratified):
    v, f = SR.squashed_icosphere()
    rec = SF.surface_cdf(v, f)
    cdf = rec['cdf'].cpu().numpy()
    for seed in (0, 0xfffffff1):
        ref = SR.sample(v, f, cdf, rec['total'], 0, n, n, seed, stratified)
        _same(_raw(SF, v, f, rec, 0, n, n, seed, stratified), ref, OUTS)
    got = SF.sample_surface(v, f, n, seed=7, stratified=stratified, return_face=True, return_bary=True, return_normals=True, cdf=rec)
    assert all(isinstance(x, np.ndarray) for x in got)                                  # numpy in, numpy out
    _same(dict(zip(OUTS, got)), SR.sample(v, f, cdf, rec['total'], 0, n, n, 7, stratified), OUTS)


def test_each_optional_output_may_be_null_and_first_may_be_positive(SF):
    v, f = SR.squashed_icosphere()
    rec = SF.surface_cdf(v, f)
    cdf = rec['cdf'].cpu().numpy()
    for stratified in (True, False):
        ref = SR.sample(v, f, cdf, rec['total'], 0, 65, 65, 11, stratified)
        for left_out in OUTS[1:]:
            want = tuple(k for k in OUTS[1:] if k != left_out)
            _same(_raw(SF, v, f, rec, 0, 65, 65, 11, stratified, want), ref, ('pts',) + want)
        _same(_raw(SF, v, f, rec, 0, 65, 65, 11, stratified, ()), ref, ('pts',))
        for first, n, n_total in ((1000, 97, 4097), (4096, 1, 4097), (1, 64, 65)):
            ref = SR.sample(v, f, cdf, rec['total'], first, n, n_total, 11, stratified)
            _same(_raw(SF, v, f, rec, first, n, n_total, 11, stratified), ref, OUTS)
    # a keyword at a time through the module: the tuple holds what was asked for, in the header's order
    ref = SR.sample(v, f, cdf, rec['total'], 0, 65, 65, 0, True)
    assert np.array_equal(SF.sample_surface(v, f, 65), ref['pts'])
    p, b = SF.sample_surface(v, f, 65, return_bary=True)
    assert np.array_equal(p, ref['pts']) and np.array_equal(b, ref['bary'])


def test_chunking_and_reruns_give_the_same_bits(SF):
    v, f = SR.squashed_icosphere()
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    for stratified in (True, False):
        kw = dict(seed=5, stratified=stratified, return_face=True, return_bary=True, return_normals=True)
        whole = SF.sample_surface(vt, ft, 4097, **kw)
        assert all(torch.is_tensor(x) and x.is_cuda for x in whole)                     # device tensors in, device tensors out
        for other in (SF.sample_surface(vt, ft, 4097, chunk=1000, **kw), SF.sample_surface(vt, ft, 4097, chunk=63, **kw),
                      SF.sample_surface(vt, ft, 4097, **kw)):
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(whole, other))
        assert not torch.equal(whole[0], SF.sample_surface(vt, ft, 4097, seed=6, stratified=stratified))


def test_degenerate_triangles_are_never_chosen_and_no_area_is_refused(SF):
    v, f, good = SR.degenerate_mesh()
    rec = SF.surface_cdf(v, f)
    cdf = rec['cdf'].cpu().numpy()
    for stratified in (True, False):
        got = _raw(SF, v, f, rec, 0, 4097, 4097, 2, stratified)
        _same(got, SR.sample(v, f, cdf, rec['total'], 0, 4097, 4097, 2, stratified), OUTS)
        assert set(got['face'].tolist()) == set(good) and np.isfinite(got['pts']).all()
    flat = f[[0, 2, 3, 6]]
    none = SF.surface_cdf(v, flat)
    assert none['total'] == 0 and none['zero_weight'] == 4 and none['area'] == 0 and not bool(none['cdf'].any())
    got = _raw(SF, v, flat, none, 0, 65, 65, 0, True)
    assert np.all(got['face'] == -1) and not any(got[k].any() for k in ('pts', 'bary', 'normal'))
    with pytest.raises(ValueError, match='no area'):
        SF.sample_surface(v, flat, 10)
    with pytest.raises(ValueError):
        SF.sample_surface(v, np.zeros((0, 3), np.int32), 10)


def test_points_lie_on_their_faces(SF):
    """with the REPORTED weights (b1, b2) -- fp32 roundings of float64 values below 1, each off by at most 2^-25 -- the mix (1 - b1 - b2) p0 +
    b1 p1 + b2 p2 in float64 differs from the stored point by at most (2 + 1 + 1) 2^-25 * 0.5 (the errors of the three weights on
    coordinates <= 0.5) + 2^-26 (the point's own rounding to fp32 at a magnitude <= 0.5) = 5 * 2^-26 = 7.5e-8 per axis; asserted below
    1e-7.  Every radius on the icosphere of radius 0.5 lies between its inscribed radius and 0.5."""
    from nero_amd.synthetic import icosphere
    v, f = icosphere(2, 0.5)
    pts, face, bary = SF.sample_surface(v, f, 4097, seed=1, stratified=False, return_face=True, return_bary=True)
    p = v.astype(np.float64)[f[face].astype(np.int64)]
    b1, b2 = bary[:, 0:1].astype(np.float64), bary[:, 1:2].astype(np.float64)
    mix = (1.0 - b1 - b2) * p[:, 0] + b1 * p[:, 1] + b2 * p[:, 2]
    err = float(np.abs(mix - pts).max())
    r = np.linalg.norm(pts.astype(np.float64), axis=1)
    print('mix error', err, 'radii', float(r.min()), float(r.max()))
    assert err < 1e-7
    assert bary.min() >= 0 and float((bary[:, 0] + bary[:, 1]).max()) <= 1.0 + 2.0 ** -23
    assert 0.491 <= r.min() and r.max() <= 0.5


def test_eval_meshes_and_the_command_line(SF, tmp_path):
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    from nero_amd.synthetic import icosphere
    pr, gt = icosphere(4, 0.5), icosphere(3, 0.5)
    c = E.eval_meshes(pr, gt, n=20000)
    assert np.isfinite(c) and c > 0
    assert c < E.eval_point_clouds(pr[0], gt[0])                   # the vertex sets are sparse on the coarse mesh: their Chamfer is larger
    assert E.eval_meshes(pr, gt, n=20000) == c
    assert E.eval_meshes(pr, gt, n=20000, seed=1) != c
    a, b = str(tmp_path / 'pr.ply'), str(tmp_path / 'gt.ply')
    M.write_ply(a, *pr)
    M.write_ply(b, *gt)
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_shape.py'), '--pr', a, '--gt', b, '--samples', '20000'],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.split() == ['pr', f'{c:.5f}']
