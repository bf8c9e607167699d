"""GPU tier: every entry point of nero_amd/csrc/sampler.hip called directly through the C ABI against tests/sampler_ref.py (pinned by
tests/test_sampler_ref_cpu.py), at the smallest shapes that cross each boundary of the kernels: the (i, i + 64) lane layout of the
wave-per-ray kernels (n = 64 / 65 / 128), the switch to the thread-per-ray kernels (n = 129; T = 193 for render_prep), the last partial
workgroup (4 rays per workgroup in the wave kernels, 64 in the thread kernels), and the production addressing (ldz = T > n, lds = n_in > n,
sdf_new at stride 4, a `variance` pointer).  Integer outputs and copies are exact; every float bound carries its origin.  Output buffers
are filled with a sentinel and carry guard rows / columns that must stay untouched."""
import ctypes as C
import functools

import pytest
import torch

from tests import sampler_ref as SR
from tests.helpers import parity_report

pytestmark = pytest.mark.gpu
P = C.c_void_p
U = SR.U
SENT, ISENT = -12345.0, -7

WAVE_R = (1, 3, 4, 5, 67)               # 4 rays per workgroup
THREAD_R = (1, 63, 65, 130)             # 64 rays per workgroup
NM_WAVE = [(2, 1), (2, 32), (3, 5), (64, 16), (65, 16), (65, 32), (127, 9), (128, 32)]
NM_THREAD = [(129, 1), (129, 31), (144, 16), (160, 32)]
NM_MERGE_WAVE = [(2, 1), (63, 1), (64, 16), (65, 32), (128, 32)]
NM_MERGE_THREAD = [(129, 31), (150, 10)]


def _lib():
    from nero_amd import _lib as L
    return L


def _p(t):
    return P(None if t is None else t.data_ptr())


_ALIVE = []


def _cu(t):
    """device copy of an input, kept alive until the test ends (the calls below take raw pointers)"""
    _ALIVE.append(t.contiguous().cuda())
    return _ALIVE[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _f(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device='cuda')


def _i(*shape):
    return torch.full(shape, ISENT, dtype=torch.int32, device='cuda')


def _untouched(t):
    return bool((t == (ISENT if t.dtype == torch.int32 else SENT)).all())


def _rel(a, b):
    """the project's relative error (tests/test_shape_render.py): max|a - b| / max|b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _rlist(n):
    return WAVE_R if n <= 128 else THREAD_R


# ---- 1. nero_sample_pdf ------------------------------------------------------------------------------------------------------------
def _sample_pdf(z, w, n, m, R, ldb=None, ldw=None, want_inds=True):
    """-> samples [R,m] (cpu), inds or None; the guard rows past R are asserted here"""
    L = _lib()
    ldb, ldw = ldb or n, ldw or n - 1
    zb, wb = _f(R, ldb), _f(R, ldw)
    zb[:, :n], wb[:, :n - 1] = z[:R].cuda(), w[:R].cuda()
    out, inds = _f(R + 2, m), _i(R + 2, m) if want_inds else None
    L.check(L.lib.nero_sample_pdf(_p(zb), ldb, _p(wb), ldw, n, m, R, _p(out), _p(inds), L.stream_ptr()))
    assert _untouched(out[R:]) and (inds is None or _untouched(inds[R:]))
    return out[:R].cpu(), None if inds is None else inds[:R].cpu()


@functools.lru_cache(maxsize=None)
def _pdf_inputs(n, m):
    """the three-spikes rows (those reaching the small-denominator branch first), an all-zero-weights row, dense random weights"""
    R = max(_rlist(n))
    z, w = SR.spike_rows(R, n, m)
    g = torch.Generator().manual_seed(11)
    w[R // 2:] = torch.rand(R - R // 2, n - 1, generator=g)
    if R > 2:
        w[2] = 0.0
    zn, inds = SR.sample_pdf_det(z, w, m)
    return z, w, zn, inds.int()


@pytest.mark.parametrize('n,m', NM_WAVE + NM_THREAD)
def test_sample_pdf_indices_exact_and_layout_invariant(n, m):
    z, w, zn_ref, inds_ref = _pdf_inputs(n, m)
    if (n, m) in ((160, 32), (128, 32), (65, 32)):
        # the inputs reach `denom < 1e-5 -> 1` (tests/test_sampler_ref_cpu.py pins the recipe)
        assert SR.small_denominators(z[:5], w[:5], m) > 0
    for R in _rlist(n):
        out, inds = _sample_pdf(z, w, n, m, R)
        if R == z.shape[0]:
            parity_report(f'sampler_kernels::sample_pdf[n={n},m={m}]', sample_max_err=float((out - zn_ref).abs().max()),
                          index_mismatches=int((inds != inds_ref).sum()))
        assert torch.equal(inds, inds_ref[:R]), (R, int((inds != inds_ref[:R]).sum()))
        # 2e-6: the project's bound on teacher-forced samples (tests/test_shape_render.py::test_sampler_stagewise_teacher_forced)
        assert float((out - zn_ref[:R]).abs().max()) < 2e-6, (R, float((out - zn_ref[:R]).abs().max()))
        out2, _ = _sample_pdf(z, w, n, m, R, want_inds=False)
        assert torch.equal(out2, out)                                   # inds_out = NULL: the same samples, bitwise
        out3, inds3 = _sample_pdf(z, w, n, m, R, ldb=n + 3, ldw=n + 1)  # padded rows: bitwise the dense call
        assert torch.equal(out3, out) and torch.equal(inds3, inds)


# ---- 2. nero_upsample --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _upsample_inputs(n):
    """rays through the unit sphere (non-unit d), sorted z across it, an SDF with a sign change; rows r % 5 == 4 never enter the unit
    sphere; rows r % 4 == 1 (n >= 3) hold a repeated z with an SDF drop: a section slope below the -1e3 clamp"""
    R = max(_rlist(n))
    g = torch.Generator().manual_seed(100 + n)
    o, d, near, far = SR.rays_through_sphere(R, g)
    z = torch.sort(near + (far - near) * torch.rand(R, n, generator=g), -1)[0]
    out = torch.arange(R) % 5 == 4
    z[out] = torch.sort(0.3 * torch.rand(int(out.sum()), n, generator=g), -1)[0] / torch.linalg.norm(d[out], dim=-1, keepdim=True)
    radius = torch.linalg.norm(o[:, None, :] + d[:, None, :] * z[..., None], dim=-1)
    sdf = radius - 0.5 + 0.02 * torch.randn(R, n, generator=g)
    if n >= 3:
        for r in range(1, R, 4):
            k = 1 + r % (n - 2)
            z[r, k] = z[r, k - 1]
            sdf[r, k] = sdf[r, k - 1] - 0.05
    return o, d, z, sdf


def _upsample(o, d, z, sdf, n, m, R, cap=64.0, variance=None, ldz=None, lds=None):
    L = _lib()
    ldz, lds = ldz or n, lds or n
    zb, sb = _f(R, ldz), _f(R, lds)
    zb[:, :n], sb[:, :n] = z[:R].cuda(), sdf[:R].cuda()
    z_new, w, inds = _f(R + 1, m), _f(R + 1, n - 1), _i(R + 1, m)
    var = None if variance is None else torch.tensor([variance], dtype=torch.float32, device='cuda')
    L.check(L.lib.nero_upsample(_p(_cu(o[:R])), _p(_cu(d[:R])), _p(zb), ldz, _p(sb), lds, n, _p(var), C.c_float(cap), m, R,
                                _p(z_new), _p(w), _p(inds), L.stream_ptr()))
    assert _untouched(z_new[R:]) and _untouched(w[R:]) and _untouched(inds[R:])
    assert _untouched(zb[:, n:]) and _untouched(sb[:, n:])
    return z_new[:R].cpu(), w[:R].cpu(), inds[:R].cpu()


@functools.lru_cache(maxsize=None)
def _upsample_run(n, m):
    """the dense call on all rows + the reference of the same inputs (shared by the per-shape test and the pooled index share)"""
    o, d, z, sdf = _upsample_inputs(n)
    R = z.shape[0]
    w_ref = SR.upsample_weights(o, d, z, sdf, 64.0)
    _, inds_ref = SR.sample_pdf_det(z, w_ref, m)
    return _upsample(o, d, z, sdf, n, m, R), w_ref, inds_ref.int()


@pytest.mark.parametrize('n,m', NM_WAVE + NM_THREAD)
def test_upsample_weights_layouts_and_variance(n, m):
    o, d, z, sdf = _upsample_inputs(n)
    Rmax = z.shape[0]
    cos, inside = SR.upsample_parts(o, d, z, sdf)
    assert bool((~inside).all(-1).any()) or Rmax < 5                    # rays that never enter the unit sphere
    if n >= 3:
        assert bool((cos < -1e3).any()) and bool((~inside).any()) and bool(inside.any())
        assert bool(((sdf[:, 1:] > 0) != (sdf[:, :-1] > 0)).any())      # a sign change of the SDF
    (z_new, w, inds), w_ref, _ = _upsample_run(n, m)
    parity_report(f'sampler_kernels::upsample[n={n},m={m}]', w_rel=_rel(w, w_ref))
    for R in _rlist(n):
        if R != Rmax:
            zr, wr, ir = _upsample(o, d, z, sdf, n, m, R)
            assert torch.equal(zr, z_new[:R]) and torch.equal(wr, w[:R]) and torch.equal(ir, inds[:R])   # a ray does not depend on R
        # 2e-5: the project's bound on the up-sampling weights (tests/test_shape_render.py::test_sampler_stagewise_teacher_forced)
        assert _rel(w[:R], w_ref[:R]) < 2e-5, (R, _rel(w[:R], w_ref[:R]))
        # its own weights through nero_sample_pdf: the same samples and indices, bitwise
        out, inds2 = _sample_pdf(z, w, n, m, R)
        assert torch.equal(out, z_new[:R]) and torch.equal(inds2, inds[:R])
    # the production layout (ldz = T > n, lds = n_in > n): bitwise the dense call
    zl, wl, il = _upsample(o, d, z, sdf, n, m, Rmax, ldz=n + 40, lds=n + 7)
    assert torch.equal(zl, z_new) and torch.equal(wl, w) and torch.equal(il, inds)
    # variance pointer, capped side: exp(10 * 0.6) = 403 > 64 -> bitwise the call without it
    zc, wc, ic = _upsample(o, d, z, sdf, n, m, Rmax, variance=0.6, ldz=n + 40, lds=n + 7)
    assert torch.equal(zc, z_new) and torch.equal(wc, w) and torch.equal(ic, inds)
    # uncapped side: inv_s = float32(exp(10 * 0.3)) ~ 20.09 < 64; the same 2e-5
    inv_s = float(torch.exp(torch.tensor(0.3, dtype=torch.float32) * 10.0))
    assert inv_s < 64.0
    _, wv, _ = _upsample(o, d, z, sdf, n, m, Rmax, variance=0.3)
    w_ref_v = SR.upsample_weights(o, d, z, sdf, inv_s)
    assert _rel(wv, w_ref_v) < 2e-5, _rel(wv, w_ref_v)
    assert _rel(w_ref_v, w_ref) > 1e-3                                   # (the two inv_s are told apart by this bound)


def test_upsample_indices_from_own_weights():
    """indices from the kernel's own weights differ from the reference's only where a 1-ulp weight difference crosses a cdf edge: the
    project's share < 2e-3 (tests/test_shape_render.py), pooled over the whole shape matrix (a single shape has too few samples for a share)"""
    bad = total = 0
    for n, m in NM_WAVE + NM_THREAD:
        (_, _, inds), _, inds_ref = _upsample_run(n, m)
        bad += int((inds != inds_ref).sum())
        total += inds.numel()
    parity_report('sampler_kernels::upsample_indices_from_own_weights', mismatches=bad, samples=total)
    assert bad / total < 2e-3, (bad, total)


# ---- 3. nero_merge_sorted ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merge_inputs(n, m):
    R = max(_rlist(n))
    z, zn = SR.tie_merge_inputs(R, n, m)
    g = torch.Generator().manual_seed(200 + n)
    for r in range(R):
        if r % 7 == 1:
            zn[r] = torch.sort(z[r, 0] - 0.1 - torch.rand(m, generator=g))[0]       # entirely below the old range
        elif r % 7 == 2:
            zn[r] = torch.sort(z[r, -1] + 0.1 + torch.rand(m, generator=g))[0]      # entirely above it
    sdf, sdf_new = torch.randn(R, n, generator=g), torch.randn(R, m, generator=g)
    zs, s, index = SR.merge_sorted(z, sdf, zn, sdf_new)
    assert torch.equal(s, torch.gather(torch.cat([sdf, sdf_new], -1), -1, index))
    return z, zn, sdf, sdf_new, zs, s, index.int()


@pytest.mark.parametrize('n,m', NM_MERGE_WAVE + NM_MERGE_THREAD)
def test_merge_sorted_permutation_exact(n, m):
    L = _lib()
    z, zn, sdf, sdf_new, zs_ref, s_ref, index_ref = _merge_inputs(n, m)
    assert bool((zn[:, :, None] == z[:, None, :]).any()) and bool((zn[1] < z[1, :1]).all()) or z.shape[0] < 2
    for R in _rlist(n):
        for ldz, lds, ldsn in ((n + m, n + m, 1), (n + m + 8, n + m + 5, 4)):       # dense; production: ldz = T, lds = n_in, ldsn = 4
            for with_sdf in (True, False):
                zb, sb = _f(R + 1, ldz), _f(R + 1, lds)
                zb[:R, :n], sb[:R, :n] = z[:R].cuda(), sdf[:R].cuda()
                src = _f(R * m + 1, ldsn)
                src[:R * m, 0] = sdf_new[:R].reshape(-1).cuda()
                index = _i(R + 1, n + m)
                L.check(L.lib.nero_merge_sorted(_p(zb), ldz, n, _p(sb if with_sdf else None), lds, _p(_cu(zn[:R])), m,
                                                _p(src if with_sdf else None), ldsn, R, _p(index), L.stream_ptr()))
                where = (R, ldz, with_sdf)
                assert torch.equal(zb[:R, :n + m].cpu(), zs_ref[:R]), where
                assert torch.equal(index[:R].cpu(), index_ref[:R]), where
                assert _untouched(zb[:R, n + m:]) and _untouched(zb[R:]) and _untouched(index[R:]), where
                if with_sdf:
                    assert torch.equal(sb[:R, :n + m].cpu(), s_ref[:R]), where
                    assert _untouched(sb[:R, n + m:]) and _untouched(sb[R:]), where
                else:
                    assert torch.equal(sb[:R, :n].cpu(), sdf[:R]) and _untouched(sb[:R, n:]) and _untouched(sb[R:]), where
                assert _untouched(src[:, 1:]) and _untouched(src[R * m:]), where


# ---- 4. nero_coarse_z / nero_background_z / nero_occ_z -----------------------------------------------------------------------------
@pytest.mark.parametrize('R,n', [(1, 1), (3, 2), (5, 63), (67, 64), (4, 65), (7, 160)])
@pytest.mark.parametrize('jitter', [False, True])
def test_coarse_z(R, n, jitter):
    L = _lib()
    g = torch.Generator().manual_seed(300 + n)
    near = 0.5 + 1.5 * torch.rand(R, 1, generator=g)
    far = near + 1.0 + 2.0 * torch.rand(R, 1, generator=g)
    rand1 = torch.rand(R, 1, generator=g) if jitter else None
    col0, ldz = 3, n + 8                                                 # the window starts at column 3 of a wider table
    buf = _f(R + 1, ldz)
    L.check(L.lib.nero_coarse_z(_p(_cu(near)), _p(_cu(far)), _p(None if rand1 is None else _cu(rand1)), R, n,
                                P(buf.data_ptr() + 4 * col0), ldz, L.stream_ptr()))
    assert _untouched(buf[:R, :col0]) and _untouched(buf[:R, col0 + n:]) and _untouched(buf[R:])
    got = buf[:R, col0:col0 + n].cpu().double()
    n64, f64 = near.double(), far.double()
    ref = SR.coarse_z(n64, f64, n, None if rand1 is None else rand1.double())
    jit = 0.0 if rand1 is None else (rand1.double() - 0.5) * 2.0 / n
    # float32 roundings of near + (far - near) * lin_i: step = 1/(n-1), step * i, (1 - .) -> lin_i to 3 x 2^-24 absolute; far - near,
    # the product, the sum: 6 roundings, each of a value no larger than M = max(|near|, |far|, |far - near|)
    M = torch.maximum(torch.maximum(n64.abs(), f64.abs()), (f64 - n64).abs())
    count = 6
    if jitter:
        # + (rand1 - 0.5), / n, the last sum (* 2 is exact): 9 roundings, of values no larger than max(M, |z|, 1)
        M = torch.maximum(torch.maximum(M, ref.abs().max(-1, keepdim=True)[0]), torch.ones_like(M))
        count = 9
    bound = count * U * M
    err = (got - ref).abs()
    parity_report(f'sampler_kernels::coarse_z[R={R},n={n},jitter={jitter}]', err_over_bound=float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    # column order: the first column is near (+ jitter), the last is far (+ jitter)
    assert bool(((got[:, :1] - (n64 + jit)).abs() <= bound).all())
    assert n == 1 or bool(((got[:, -1:] - (f64 + jit)).abs() <= bound).all())


def _background_terms(nb, rand_bg):
    """float64 zo (flipped to the output order), and the stratum ends (lower, upper) of the jittered form"""
    zo = torch.linspace(1e-3, 1.0 - 1.0 / (nb + 1.0), nb, dtype=torch.float64)
    mids = 0.5 * (zo[1:] + zo[:-1])
    lower, upper = torch.cat([zo[:1], mids]), torch.cat([mids, zo[-1:]])
    if rand_bg is not None:
        zo = lower[None, :] + (upper - lower)[None, :] * rand_bg
    else:
        zo = zo[None, :]
    return torch.flip(zo, [-1]), torch.flip(lower, [-1])[None, :], torch.flip(upper, [-1])[None, :]


@pytest.mark.parametrize('R,nb', [(5, 1), (3, 2), (67, 8), (4, 32), (9, 33)])
@pytest.mark.parametrize('jitter', [False, True])
def test_background_z(R, nb, jitter):
    L = _lib()
    g = torch.Generator().manual_seed(400 + nb)
    far = 2.0 + 2.0 * torch.rand(R, 1, generator=g)
    rand_bg = torch.rand(R, nb, generator=g) if jitter else None
    col0, ldz = 5, nb + 9
    buf = _f(R + 1, ldz)
    L.check(L.lib.nero_background_z(_p(_cu(far)), _p(None if rand_bg is None else _cu(rand_bg)), R, nb, _p(buf), ldz, col0, L.stream_ptr()))
    assert _untouched(buf[:R, :col0]) and _untouched(buf[:R, col0 + nb:]) and _untouched(buf[R:])
    got = buf[:R, col0:col0 + nb].cpu().double()
    rb = None if rand_bg is None else rand_bg.double()
    ref = SR.background_z(far.double(), nb, rb)
    zo, lower, upper = _background_terms(nb, rb)
    # far / zo + 1/n_bg is a chain of positive terms: relative errors add.  zo = linspace(1e-3, 1 - 1/(n_bg+1))[k] in float32:
    #   `end` 3 roundings of values <= 1, the constant 1e-3f 1; step = (end - start) / (n_bg - 1): (3 + 1 + 1) / (end - start >= 0.5) + 1;
    #   first half  start + step * k : no cancellation, relative 8.4 -> 11 x 2^-24;
    #   second half end - step * j   : absolute 3 + 7.4 * 0.5 + 1 = 7.7 x 2^-24 of a value >= 1/3 -> relative 23; bounded by 36 x 2^-24.
    # then far / zo, 1 / n_bg and the sum: 3 more roundings -> 39 x 2^-24 relative.
    rel = 39 * U * torch.ones_like(ref)
    if jitter:
        #   lower / upper = 0.5 * (zo + neighbour): 36 + 1 = 37 relative each; upper - lower CANCELS: absolute 37 (upper + lower) + 1 (upper - lower);
        #   * rand (<= 1) + 1; lower + .: zo' to (37 lower + 76 upper + zo') x 2^-24 absolute, i.e. relative to zo' -- large where rand is small
        #   in the first stratum (lower = 1e-3, upper = 64 x that at n_bg = 8); then the same 3 roundings
        rel = ((37 * lower + 76 * upper + zo) / zo + 3) * U
    bound = rel * ref
    err = (got - ref).abs()
    parity_report(f'sampler_kernels::background_z[R={R},nb={nb},jitter={jitter}]', err_over_bound=float((err / bound).max()),
                  rel_err=float((err / ref).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    # column order: zo is flipped, z ascends along the row (the strata do not overlap), the first column is the far end of zo
    assert bool((got[:, 1:] > got[:, :-1]).all())
    if not jitter:
        end = 1.0 - 1.0 / (nb + 1.0) if nb > 1 else 1e-3
        assert bool(((got[:, :1] - (far.double() / end + 1.0 / nb)).abs() <= bound[:, :1]).all())
        assert bool(((got[:, -1:] - (far.double() / 1e-3 + 1.0 / nb)).abs() <= bound[:, -1:]).all())


@pytest.mark.parametrize('Pn,n', [(1, 1), (1, 2), (5, 64), (67, 16), (3, 65)])
def test_occ_z(Pn, n):
    """(the entry point takes a dense [P,n] table: no ldz / col0, and no random draw, to vary)"""
    L = _lib()
    g = torch.Generator().manual_seed(500 + n)
    o = torch.nn.functional.normalize(torch.randn(Pn, 3, generator=g), dim=-1) * 0.8 * torch.rand(Pn, 1, generator=g)
    d = torch.nn.functional.normalize(torch.randn(Pn, 3, generator=g), dim=-1)
    buf = _f(Pn + 1, n)
    L.check(L.lib.nero_occ_z(_p(_cu(o)), _p(_cu(d)), Pn, n, _p(buf), L.stream_ptr()))
    assert _untouched(buf[Pn:])
    got = buf[:Pn].cpu().double()
    ref = SR.occ_z(o.double(), d.double(), n)
    # |o| <= 0.8, |d| = 1: every intermediate is below M = 2 (disc = dtx^2 - xtx + 1 + 1e-6 <= 1.65, maxd <= 1.8) and disc >= 0.36, so the
    # square root passes absolute errors on with a factor 1 / (2 sqrt(disc)) <= 0.84.  Roundings: dtx 5, xtx 5; dtx*dtx carries 2|dtx| x 5 = 8
    # + 1; - xtx 5 + 1; + 1, + 1e-6: 2 -> disc to 17; sqrt: 17 x 0.84 + 2 -> 17; -dtx + .: 5 + 17 + 1 = 23; lin_i to 3 (x maxd <= 1.8 -> 6)
    # and the product 1: 30 roundings x 2^-24 x M
    assert float(torch.linalg.norm(o, dim=-1).max()) <= 0.8 + 1e-6
    bound = 30 * U * 2.0
    parity_report(f'sampler_kernels::occ_z[P={Pn},n={n}]', err_over_bound=float((got - ref).abs().max()) / bound)
    assert float((got - ref).abs().max()) <= bound, float((got - ref).abs().max()) / bound
    assert float(got[:, 0].abs().max()) == 0.0                           # the march starts at the point itself


# ---- 5. nero_scatter_sdf -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,n', [(1, 1), (5, 63), (67, 16), (3, 160)])
def test_scatter_sdf(R, n):
    L = _lib()
    g = torch.Generator().manual_seed(600 + n)
    src = torch.randn(R * n, 4, generator=g)
    lds = n + 6
    tab = _f(R + 1, lds)
    L.check(L.lib.nero_scatter_sdf(_p(_cu(src)), 4, R, n, _p(tab), lds, L.stream_ptr()))
    assert torch.equal(tab[:R, :n].cpu(), src[:, 0].reshape(R, n))
    assert _untouched(tab[:R, n:]) and _untouched(tab[R:])


# ---- 6. / 7. nero_render_prep (+ the scan), nero_compact ---------------------------------------------------------------------------
def _prep_inputs(R, T, seed, kind='mixed'):
    """rays from distance 2.5 .. 3 through the unit sphere, z sorted across it.  kind 'mixed': rows r % 6 == 5 stay in front of the sphere
    (count 0), rows r % 6 == 4 are short rays near the origin (count T); 'outside' / 'inside': every row of that kind"""
    g = torch.Generator().manual_seed(seed)
    o, d, near, far = SR.rays_through_sphere(R, g)
    span = far - near
    z = torch.sort(near - 0.3 * span + 1.6 * span * torch.rand(R, T, generator=g), -1)[0]
    r = torch.arange(R)
    front = (r % 6 == 5) if kind == 'mixed' else torch.full((R,), kind == 'outside')
    short = (r % 6 == 4) if kind == 'mixed' else torch.full((R,), kind == 'inside')
    z[front] = torch.sort(0.3 * torch.rand(int(front.sum()), T, generator=g), -1)[0] / torch.linalg.norm(d[front], dim=-1, keepdim=True)
    ns = int(short.sum())
    o[short] = 0.3 * (2 * torch.rand(ns, 3, generator=g) - 1) / 3 ** 0.5
    d[short] = torch.nn.functional.normalize(torch.randn(ns, 3, generator=g), dim=-1) * 0.4 * torch.rand(ns, 1, generator=g)
    z[short] = torch.sort(torch.rand(ns, T, generator=g), -1)[0]
    return o, d, z


def _render_prep(o, d, z):
    L = _lib()
    R, T = z.shape
    pts4, rc, ro, counts = _f(R * T + 3, 4), _i(R + 2), _i(R + 2), _i(3)
    L.check(L.lib.nero_render_prep(_p(_cu(o)), _p(_cu(d)), _p(_cu(z)), R, T, _p(pts4), _p(rc), _p(ro), _p(counts), L.stream_ptr()))
    assert _untouched(pts4[R * T:]) and _untouched(rc[R:]) and _untouched(ro[R:]) and _untouched(counts[2:])
    return pts4[:R * T].cpu(), rc[:R].cpu().long(), ro[:R].cpu().long(), counts[:2].cpu().long()


def _check_prep(o, d, z, tag):
    R, T = z.shape
    pts4, rc, ro, counts = _render_prep(o, d, z)
    # pts4 is a float32 elementwise expression compiled without contraction: the float32 torch statement, bit for bit
    assert torch.equal(pts4, SR.render_prep_f32(o, d, z)), tag
    ref = SR.render_prep(o.double(), d.double(), z.double())
    # samples whose float64 radius (of the kernel's own points) is within 1e-6 of the sphere may fall on either side: left out, at most 0.1 %
    band = ((torch.linalg.norm(pts4[:, :3].double(), dim=-1) - 1.0).abs() < 1e-6).reshape(R, T)
    share = float(band.double().mean())
    assert share <= 1e-3, (tag, share)
    clear = ~band.any(-1)
    assert torch.equal(rc[clear], ref['ray_counts'][clear]), tag
    assert bool(((rc - ref['ray_counts']).abs() <= band.sum(-1)).all()), tag
    assert torch.equal(ro, SR.exclusive_offsets(rc)), tag
    assert counts.tolist() == [int(rc.sum()), R * T - int(rc.sum())], tag
    return pts4, rc, ro, share, ref


@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 160, 192, 193, 200])
def test_render_prep_points_counts_offsets(T):
    """T = 2 .. 192: one wavefront per ray; T = 1, 193, 200: one thread per ray -- each compared with the reference, not with the other"""
    rlist = WAVE_R if 2 <= T <= 192 else THREAD_R
    worst = 0.0
    for R in rlist:
        o, d, z = _prep_inputs(R, T, seed=700 + T)
        _, rc, _, share, ref = _check_prep(o, d, z, (T, R))
        worst = max(worst, share)
        if R >= 6:
            assert bool((ref['ray_counts'] == 0).any()) and bool((ref['ray_counts'] == T).any())
            assert bool((rc == 0).any()) and bool((rc == T).any())
    parity_report(f'sampler_kernels::render_prep[T={T}]', band_share=worst, rays=list(rlist))


@pytest.mark.parametrize('R', [1, 1023, 1024, 1025, 3000])
def test_ray_scan_offsets(R):
    """the single-workgroup scan over many rays (1024 threads, ceil(R / 1024) rays each), with rays of count 0 and of count T"""
    o, d, z = _prep_inputs(R, 2, seed=800 + R)
    _, rc, _, share, _ = _check_prep(o, d, z, ('scan', R))
    assert R < 6 or (bool((rc == 0).any()) and bool((rc == 2).any()))
    parity_report(f'sampler_kernels::ray_scan[R={R}]', band_share=share)


@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 160, 192, 193, 200])
@pytest.mark.parametrize('kind', ['mixed', 'outside', 'inside'])
def test_compact_order(T, kind):
    L = _lib()
    for R in WAVE_R if kind == 'mixed' else (5,):
        o, d, z = _prep_inputs(R, T, seed=900 + T, kind=kind)
        pts4 = SR.render_prep_f32(o, d, z)
        mask = SR.inner_mask_f32(pts4)                                  # the kernel's own predicate, in float32 torch
        per_ray = mask.reshape(R, T).sum(-1)
        n_in, n_out = int(mask.sum()), R * T - int(mask.sum())
        if kind != 'mixed':
            assert (n_in == 0) if kind == 'outside' else (n_out == 0)   # an empty partition
        inner, outer = _i(n_in + 2), _i(n_out + 2)
        ray_off = _cu(SR.exclusive_offsets(per_ray).int())
        L.check(L.lib.nero_compact(_p(_cu(pts4)), _p(ray_off), R, T, _p(inner), _p(outer), L.stream_ptr()))
        assert _untouched(inner[n_in:]) and _untouched(outer[n_out:])
        ii, oi = SR.compact(mask)
        # rays holding a sample within 1e-6 of the sphere are left out (at most 0.1 % of the samples are such)
        band = ((torch.linalg.norm(pts4[:, :3].double(), dim=-1) - 1.0).abs() < 1e-6).reshape(R, T)
        assert float(band.double().mean()) <= 1e-3
        clear = ~band.any(-1)
        assert torch.equal(inner[:n_in].cpu().long()[clear[ii // T]], ii[clear[ii // T]]), (T, R, kind)
        assert torch.equal(outer[:n_out].cpu().long()[clear[oi // T]], oi[clear[oi // T]]), (T, R, kind)


# ---- 8. / 9. the gathers and the ray-point encoder ---------------------------------------------------------------------------------
def _check_pe(rows, n, raw, n_freq, width, tag):
    """rows [pad + guard, ld] from a PE kernel: raw columns == `raw` bitwise, zero pad columns, zero rows n .. pad-1, untouched guard rows;
    sin / cos columns within 2e-5 of the float64 reference rows built from the row's OWN raw columns (a 1-ulp difference of the argument is
    multiplied by up to 2^9; where the raw columns are computed in the kernel the caller bounds them against float64).  -> the measured maximum"""
    pad, dim = SR.row_pad(n), raw.shape[1]
    rows_c = rows.cpu()
    assert _untouched(rows[pad:]), tag
    assert float(rows_c[n:pad].abs().max()) == 0.0 if pad > n else True, tag
    assert float(rows_c[:pad, width:].abs().max()) == 0.0, tag
    assert torch.equal(rows_c[:n, :dim], raw), tag
    ref = {6: SR.pe6_rows, 10: SR.pe10_rows88, 4: SR.pe4_rows32}[n_freq](rows_c[:n, :dim].double(), pad)
    assert ref.shape == rows_c[:pad].shape and width == dim * (1 + 2 * n_freq), tag
    err = float((rows_c[:pad].double() - ref).abs().max())
    # 2e-5: the project's bound on device sin / cos of float32 arguments up to 2^9 |x| (tests/test_units_gpu.py)
    assert err < 2e-5, (tag, err)
    return err


@functools.lru_cache(maxsize=None)
def _gather_table():
    """a [R*T, 4] sample table (points at radius 0.3 .. 3, w = section length) and R distinct non-unit ray directions"""
    g = torch.Generator().manual_seed(1000)
    R, T = 40, 7
    p = torch.nn.functional.normalize(torch.randn(R * T, 3, generator=g), dim=-1) * (0.3 + 2.7 * torch.rand(R * T, 1, generator=g))
    pts4 = torch.cat([p, 0.01 + torch.rand(R * T, 1, generator=g)], -1)
    d = torch.randn(R, 3, generator=g) * (0.5 + torch.rand(R, 1, generator=g))
    return R, T, pts4, d


@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_gather_inner(n):
    L = _lib()
    R, T, pts4, _ = _gather_table()
    g = torch.Generator().manual_seed(1100 + n)
    idx = torch.sort(torch.randperm(R * T, generator=g)[:n])[0].int()
    pad = SR.row_pad(n)
    x4, pe = _f(pad + 2, 4), _f(pad + 2, 40)
    L.check(L.lib.nero_gather_inner(_p(_cu(pts4)), _p(_cu(idx)), n, _p(x4), _p(pe), L.stream_ptr()))
    want = pts4[idx.long()]
    assert torch.equal(x4[:n].cpu(), want) and _untouched(x4[pad:])
    assert float(x4[n:pad].abs().max()) == 0.0 if pad > n else True
    err = _check_pe(pe, n, want[:, :3], 6, 39, ('gather_inner', n))
    parity_report(f'sampler_kernels::gather_inner[n={n}]', pe6_max_err=err)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_gather_outer(n):
    L = _lib()
    R, T, pts4, d = _gather_table()
    g = torch.Generator().manual_seed(1200 + n)
    idx = torch.sort(torch.randperm(R * T, generator=g)[:n])[0].int()
    pad = SR.row_pad(n)
    pe88, pev32, dist = _f(pad + 2, 88), _f(pad + 2, 32), _f(pad + 2)
    L.check(L.lib.nero_gather_outer(_p(_cu(pts4)), _p(_cu(d)), _p(_cu(idx)), T, n, _p(pe88), _p(pev32), _p(dist), L.stream_ptr()))
    want = pts4[idx.long()]
    assert torch.equal(dist[:n].cpu(), want[:, 3]) and _untouched(dist[pad:])
    assert float(dist[n:pad].abs().max()) == 0.0 if pad > n else True
    # raw columns: [p/|p|, 1/|p|] and -d/|d| of ray idx // T against float64.  |p|: three products and two sums of positive terms (3 x 2^-24
    # relative on the sum of squares, halved by the square root: 1.5), the root 1, the division 1, one more for a root that is faithfully rather
    # than correctly rounded: 5 roundings x 2^-24, relative to each value
    p4 = SR.outer_point(want[:, :3].double())
    raw88 = pe88[:n, :4].cpu()
    assert bool(((raw88.double() - p4).abs() <= 5 * U * p4.abs()).all()), float(((raw88.double() - p4).abs() / p4.abs()).max() / U)
    w = SR.view_dir(d.double()[idx.long() // T])
    raw32 = pev32[:n, :3].cpu()
    assert bool(((raw32.double() - w).abs() <= 5 * U * w.abs()).all()), float(((raw32.double() - w).abs() / w.abs()).max() / U)
    e88 = _check_pe(pe88, n, raw88, 10, 84, ('gather_outer pe88', n))
    e32 = _check_pe(pev32, n, raw32, 4, 27, ('gather_outer pev32', n))
    parity_report(f'sampler_kernels::gather_outer[n={n}]', pe10_max_err=e88, pe4_max_err=e32)


@pytest.mark.parametrize('R,ldz,col0,ncols', [(5, 23, 3, 13), (1, 4, 2, 1), (3, 70, 1, 64)])
def test_ray_points_pe(R, ldz, col0, ncols):
    L = _lib()
    g = torch.Generator().manual_seed(1300 + ncols)
    o, d = torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    z = 0.5 * torch.rand(R, ldz, generator=g)
    n = R * ncols
    pad = SR.row_pad(n)
    assert n % 64 != 0 or ncols == 64
    pe = _f(pad + 2, 40)
    L.check(L.lib.nero_ray_points_pe(_p(_cu(o)), _p(_cu(d)), _p(_cu(z)), ldz, col0, ncols, R, _p(pe), L.stream_ptr()))
    t = z[:, col0:col0 + ncols]
    pts = (o[:, None, :] + d[:, None, :] * t[..., None]).reshape(n, 3)      # float32, op for op (no contraction in the kernel)
    err = _check_pe(pe, n, pts, 6, 39, ('ray_points_pe', R, ncols))
    parity_report(f'sampler_kernels::ray_points_pe[R={R},ncols={ncols}]', pe6_max_err=err)


# ---- 10. nero_section_weights ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,Pn', [(2, 1), (9, 65), (128, 130)])
@pytest.mark.parametrize('lds', [4, 1])
def test_section_weights(n, Pn, lds):
    L = _lib()
    g = torch.Generator().manual_seed(1400 + n)
    z = torch.sort(1.5 * torch.rand(Pn, n, generator=g), -1)[0]
    z[:, 0] = 0.0
    sdf = 0.3 * torch.cos(3.0 * z + 6.28 * torch.rand(Pn, 1, generator=g)) + 0.01 * torch.randn(Pn, n, generator=g)
    if n > 2:
        sdf[:, 2] = sdf[:, 1]                                           # a flat section: slope exactly 0
    src = _f(Pn * n + 1, lds)
    src[:Pn * n, 0] = sdf.reshape(-1).cuda()
    var = torch.tensor([0.3], dtype=torch.float32, device='cuda')
    inv_s = float(torch.exp(torch.tensor(0.3, dtype=torch.float32) * 10.0))
    w_ref, cos = SR.section_weights(z.double(), sdf.double(), inv_s)
    w, wsum = _f(Pn + 1, max(n - 1, 1)), _f(Pn + 1)
    zc = _cu(z)
    L.check(L.lib.nero_section_weights(_p(zc), _p(src), lds, n, _p(var), Pn, _p(w), _p(wsum), L.stream_ptr()))
    wsum_only = _f(Pn + 1)
    L.check(L.lib.nero_section_weights(_p(zc), _p(src), lds, n, _p(var), Pn, _p(None), _p(wsum_only), L.stream_ptr()))
    assert _untouched(w[Pn:]) and _untouched(wsum[Pn:]) and _untouched(wsum_only[Pn:]) and _untouched(src[:, 1:]) and _untouched(src[Pn * n:])
    wc = w[:Pn, :n - 1].cpu()
    # 2e-5: the project's bound on NeuS section weights (tests/test_shape_render.py), max|a - b| / max|b|
    assert _rel(wc, w_ref) < 2e-5, _rel(wc, w_ref)
    # the sign of a slope is the sign of a float32 difference: exact in both evaluations.  Sections that do not descend weigh exactly 0
    assert bool((cos >= 0).any()) or n == 2
    assert bool((wc[cos >= 0] == 0).all())
    assert torch.equal(wsum_only[:Pn], wsum[:Pn])
    s_ref = w_ref.sum(-1)
    # a serial float32 sum of n - 1 terms, each within the 2e-5 above: (n - 1) x 2^-24 x sum + 2e-5 x sum
    bound = (n - 1) * U * s_ref + 2e-5 * s_ref
    err = (wsum_only[:Pn].cpu().double() - s_ref).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    parity_report(f'sampler_kernels::section_weights[n={n},lds={lds}]', w_rel=_rel(wc, w_ref), wsum_rel=float((err / s_ref.clamp_min(1e-30)).max()))


# ---- 11. nero_occ_candidates -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 300])
def test_occ_candidates(n):
    L = _lib()
    g = torch.Generator().manual_seed(1500 + n)
    R, T = 50, 7
    x = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * (0.9 + 0.15 * torch.rand(n, 1, generator=g))
    x4 = torch.cat([x, torch.rand(n, 1, generator=g)], -1)
    sdf4 = torch.cat([0.02 * (2 * torch.rand(n, 1, generator=g) - 1), torch.randn(n, 3, generator=g)], -1)
    grad = torch.randn(n, 3, generator=g)
    idx = torch.sort(torch.randperm(R * T, generator=g)[:n])[0].int()
    d = torch.randn(R, 3, generator=g) * (0.5 + 2.0 * torch.rand(R, 1, generator=g))     # non-unit: the kernel normalises
    flag = torch.full((n + 3,), 9, dtype=torch.uint8, device='cuda')
    L.check(L.lib.nero_occ_candidates(_p(_cu(x4)), _p(_cu(sdf4)), _p(_cu(grad)), _p(_cu(idx)), _p(_cu(d)), T, C.c_float(0.01), n, _p(flag),
                                      L.stream_ptr()))
    assert bool((flag[n:] == 9).all())
    dr = d[idx.long() // T].double()
    ref, margin = SR.occ_candidates(x.double(), sdf4[:, 0].double(), grad.double(), dr, 0.01)
    keep = margin >= 1e-6                                                # rows within a relative 1e-6 of a threshold: at most 0.1 %
    assert float((~keep).double().mean()) <= 1e-3
    if n > 1:
        rad, dot = torch.linalg.norm(x.double(), dim=-1), (grad.double() * dr).sum(-1)
        for c in (rad < 0.999, sdf4[:, 0].abs() < 0.01, dot < 0):        # every clause decides some row
            assert bool(c.any()) and bool((~c).any())
        assert bool(ref.any()) and bool((~ref).any())
        # with the unnormalised direction the third clause is the same; a wrong ray is not: the rows tell the rays apart
        assert bool((((grad.double() * d.double()[(idx.long() // T + 1) % R]).sum(-1) < 0) != (dot < 0)).any())
    assert torch.equal(flag[:n].cpu()[keep] != 0, ref[keep])
    parity_report(f'sampler_kernels::occ_candidates[n={n}]', left_out=int((~keep).sum()))


# ---- 12. argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks_reject_before_launch():
    L = _lib()
    st = L.stream_ptr()
    lib = L.lib
    R = 3
    o, d = _f(R, 3), _f(R, 3)
    z, sdf, w = _f(R, 200), _f(R, 200), _f(R, 200)
    out, inds, index = _f(R, 64), _i(R, 64), _i(R, 200)
    i3 = _i(R)
    flag = torch.full((8,), 9, dtype=torch.uint8, device='cuda')
    bad = [
        lambda: lib.nero_upsample(_p(o), _p(d), _p(z), 200, _p(sdf), 200, 1, _p(None), C.c_float(64.0), 4, R, _p(out), _p(w), _p(inds), st),
        lambda: lib.nero_upsample(_p(o), _p(d), _p(z), 200, _p(sdf), 200, 161, _p(None), C.c_float(64.0), 4, R, _p(out), _p(w), _p(inds), st),
        lambda: lib.nero_upsample(_p(o), _p(d), _p(z), 200, _p(sdf), 200, 64, _p(None), C.c_float(64.0), 33, R, _p(out), _p(w), _p(inds), st),
        lambda: lib.nero_upsample(_p(o), _p(d), _p(z), 200, _p(None), 200, 64, _p(None), C.c_float(64.0), 4, R, _p(out), _p(w), _p(inds), st),
        lambda: lib.nero_upsample(_p(o), _p(d), _p(z), 200, _p(sdf), 200, 64, _p(None), C.c_float(64.0), 4, R, _p(None), _p(w), _p(inds), st),
        lambda: lib.nero_sample_pdf(_p(z), 200, _p(w), 200, 1, 4, R, _p(out), _p(inds), st),
        lambda: lib.nero_sample_pdf(_p(z), 200, _p(w), 200, 161, 4, R, _p(out), _p(inds), st),
        lambda: lib.nero_sample_pdf(_p(z), 200, _p(w), 200, 64, 33, R, _p(out), _p(inds), st),
        lambda: lib.nero_sample_pdf(_p(z), 200, _p(None), 200, 64, 4, R, _p(out), _p(inds), st),
        lambda: lib.nero_sample_pdf(_p(z), 200, _p(w), 200, 64, 4, R, _p(None), _p(inds), st),
        lambda: lib.nero_merge_sorted(_p(z), 200, 129, _p(sdf), 200, _p(out), 32, _p(w), 1, R, _p(index), st),
        lambda: lib.nero_merge_sorted(_p(z), 200, 64, _p(sdf), 200, _p(None), 16, _p(w), 1, R, _p(index), st),
        lambda: lib.nero_merge_sorted(_p(None), 200, 64, _p(sdf), 200, _p(out), 16, _p(w), 1, R, _p(index), st),
        lambda: lib.nero_coarse_z(_p(o), _p(None), _p(None), R, 64, _p(z), 200, st),
        lambda: lib.nero_coarse_z(_p(o), _p(d), _p(None), R, 161, _p(z), 200, st),
        lambda: lib.nero_background_z(_p(None), _p(None), R, 8, _p(z), 200, 0, st),
        lambda: lib.nero_ray_points_pe(_p(o), _p(d), _p(z), 200, 0, 4, R, _p(None), st),
        lambda: lib.nero_scatter_sdf(_p(None), 4, R, 16, _p(sdf), 200, st),
        lambda: lib.nero_render_prep(_p(o), _p(d), _p(z), R, 64, _p(w), _p(i3), _p(None), _p(inds), st),
        lambda: lib.nero_render_prep(_p(o), _p(d), _p(z), R, 0, _p(w), _p(i3), _p(i3), _p(inds), st),
        lambda: lib.nero_compact(_p(w), _p(None), R, 8, _p(inds), _p(index), st),
        lambda: lib.nero_gather_inner(_p(w), _p(None), 5, _p(out), _p(z), st),
        lambda: lib.nero_gather_outer(_p(w), _p(d), _p(i3), 8, 3, _p(z), _p(None), _p(out), st),
        lambda: lib.nero_occ_candidates(_p(w), _p(sdf), _p(None), _p(i3), _p(d), 8, C.c_float(0.01), 3, _p(flag), st),
        lambda: lib.nero_occ_z(_p(o), _p(None), R, 16, _p(z), st),
        lambda: lib.nero_section_weights(_p(z), _p(sdf), 4, 16, _p(None), R, _p(w), _p(out), st),
        lambda: lib.nero_section_weights(_p(z), _p(sdf), 4, 16, _p(o), R, _p(None), _p(None), st),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.NeroHipError):
            L.check(call())
        assert 'bad argument' in L.lib.nero_last_error().decode(), k
    torch.cuda.synchronize()
    for t in (o, d, z, sdf, w, out, inds, index, i3):
        assert _untouched(t)
    assert bool((flag == 9).all())
    # no rays: OK, nothing written
    ok = [
        lib.nero_upsample(_p(o), _p(d), _p(z), 200, _p(sdf), 200, 64, _p(None), C.c_float(64.0), 4, 0, _p(out), _p(w), _p(inds), st),
        lib.nero_sample_pdf(_p(z), 200, _p(w), 200, 64, 4, 0, _p(out), _p(inds), st),
        lib.nero_merge_sorted(_p(z), 200, 64, _p(sdf), 200, _p(out), 16, _p(w), 1, 0, _p(index), st),
        lib.nero_coarse_z(_p(o), _p(d), _p(None), 0, 64, _p(z), 200, st),
        lib.nero_background_z(_p(o), _p(None), 0, 8, _p(z), 200, 0, st),
        lib.nero_ray_points_pe(_p(o), _p(d), _p(z), 200, 0, 4, 0, _p(w), st),
        lib.nero_scatter_sdf(_p(w), 4, 0, 16, _p(sdf), 200, st),
        lib.nero_render_prep(_p(o), _p(d), _p(z), 0, 64, _p(w), _p(i3), _p(i3), _p(inds), st),
        lib.nero_compact(_p(w), _p(i3), 0, 8, _p(inds), _p(index), st),
        lib.nero_gather_inner(_p(w), _p(i3), 0, _p(out), _p(z), st),
        lib.nero_gather_outer(_p(w), _p(d), _p(i3), 8, 0, _p(z), _p(sdf), _p(out), st),
        lib.nero_occ_candidates(_p(w), _p(sdf), _p(z), _p(i3), _p(d), 8, C.c_float(0.01), 0, _p(flag), st),
        lib.nero_occ_z(_p(o), _p(d), 0, 16, _p(z), st),
        lib.nero_section_weights(_p(z), _p(sdf), 4, 16, _p(o), 0, _p(w), _p(out), st),
    ]
    assert ok == [0] * len(ok)
    torch.cuda.synchronize()
    for t in (o, d, z, sdf, w, out, inds, index, i3):
        assert _untouched(t)
