"""GPU tier: every entry point of nero_amd/csrc/shade.hip, and the positional-encoding calls of encode.hip, called directly through the C ABI
against tests/shade_ref.py (pinned by tests/test_shade_ref_cpu.py), at the smallest shapes that cross each boundary of the kernels: the
128-thread blocks of the per-sample kernels, the 64-row blocks of the LDS-staged ones and the 64-row pad (n = 1 ... 200), rays and poses
picked by idx[k] / T (T = 1, 5, 160), the 64-lane chunks of the wave-per-ray compositing (T = 1 ... 192) and the thread-per-ray kernels
behind it (T = 193, 200).

Compared against: the float64 reference evaluated on the kernel's own float32 inputs, PER ROW: err(row) = max|got - ref| / max|ref| over the
row (an element of a 1-D output is its own row), never against the batch maximum.  An output that is by construction the DIFFERENCE of
larger terms is measured, per row, against the larger of its own magnitude and the size of those terms, which the reference states in
float64 from the row's inputs (`unit`: tests/shade_ref.py::sdf_alpha_term_sizes, composite_bwd_term_sizes, combine_bwd(want_lut_size)).  Integers, copies, zero pad rows and sentinel guards are
exact.  Float bounds are MEASURED: the same reference evaluated in float32 on the CPU has a worst row error against float64 -- the floor --
and the kernel gets floor_factor = 3 times it (tests/helpers.py: device expf / sinf / powf differ from the host's by ulps, and the
association order differs).  A row within ROUNDINGS = 8 float32 roundings (8 x 2^-24 of its own magnitude) is accepted whatever the floor:
no output here is fewer than eight rounded operations away from its inputs (a sigmoid alone is negate, exp, add, divide with a 1-2 ulp
exp), and a float32 CPU evaluation can be exact to the last bit by luck.  Backward references are float64 autograd of the forward
reference, so every tie is torch's.  No bound is derived from the kernel's output; every measured figure goes to parity_report."""
import ctypes as C
import functools

import pytest
import torch

from tests import shade_ref as S
from tests.helpers import parity_report, ref_fg_lut

pytestmark = pytest.mark.gpu
P = C.c_void_p
SENT, ISENT = -12345.0, -7
GUARD = 3
FLOOR_FACTOR, ROUNDINGS = 3.0, 8
TINY = 1e-300              # (only keeps 0 / 0 of an all-zero reference row from being NaN: the kernel must give exact zeros there)
F32, F64 = torch.float32, torch.float64
ANNEALS = (0.0, 0.3, 1.0)
NS = [n for n, _, _ in S.PER_SAMPLE]


def _lib():
    from nero_amd import _lib as L
    return L


def _p(t):
    return P(None if t is None else t.data_ptr())


_ALIVE = []


def _cu(t):
    """device copy of an input, kept alive until the test ends (the calls below take raw pointers)"""
    if t is None:
        return None
    _ALIVE.append(t.contiguous().cuda())
    return _ALIVE[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _f(*shape):
    t = torch.full(shape, SENT, dtype=F32, device='cuda')
    _ALIVE.append(t)
    return t


def _untouched(t):
    return bool((t == SENT).all())


def _out(n, *width, pad=False):
    """sentinel-filled output of n (pad: NERO_ROW_PAD(n)) rows + GUARD guard rows"""
    return _f((S.row_pad(n) if pad else n) + GUARD, *width)


def _take(buf, n, pad=False):
    """the n live rows (cpu); pad: rows n .. NERO_ROW_PAD(n)-1 must be zero; the guard rows behind must be untouched"""
    rows = S.row_pad(n) if pad else n
    assert _untouched(buf[rows:]), 'guard rows written'
    if pad:
        assert bool((buf[n:rows] == 0).all()), 'pad rows not zero'
    return buf[:n].cpu()


def _row_err(a, ref, unit=0.0):
    """worst row of |a - ref| / max(|ref| of the row, unit of the row); unit: a number, or per row [n] / [n,k] (the row's largest counts)"""
    a, ref = a.double().reshape(a.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    if not a.numel():
        return 0.0
    rows = ref.abs().max(-1)[0].clamp(min=TINY)
    if torch.is_tensor(unit):
        rows = torch.maximum(rows, unit.double().reshape(a.shape[0], -1).max(-1)[0])
    else:
        rows = rows.clamp(min=max(unit, TINY))
    return ((a - ref).abs().max(-1)[0] / rows).max().item()


_FLOORS = {}


def _floors(refs_fn, variant=()):
    """the float32 floor of every output of a family: the worst row of the float32 reference against the float64 one over ALL shapes of the
    family (the worst row of one shape alone is a statistic of a few hundred samples and moves by orders of magnitude from shape to shape).
    CPU only, computed once."""
    key = (refs_fn.__name__, variant)
    if key not in _FLOORS:
        out = {}
        for shape in S.PER_SAMPLE:
            for name, (r64, r32, unit) in refs_fn(*shape, *variant).items():
                out[name] = max(out.get(name, 0.0), _row_err(r32, r64, unit))
        _FLOORS[key] = out
    return _FLOORS[key]


def _judge(report, name, got, ref, floor):
    """ref = (float64 reference, float32 reference, unit); per-row distance of the kernel from the float64 reference against
    max(3 x floor, 8 roundings).  unit: for an output formed as a difference from a constant of that size (1 - exp(.), (|g| - 1)^2) a row
    is measured against at least that constant: float32 cannot resolve such a value relative to itself, in any implementation"""
    r64, r32, unit = ref
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert bool(torch.isfinite(got).all()), name
    err, own = _row_err(got, r64, unit), _row_err(r32, r64, unit)
    bound = max(FLOOR_FACTOR * floor, ROUNDINGS * S.EPS32)
    report[name] = dict(fp32_floor=floor, fp32_floor_this_shape=own, kernel=err, bound=bound,
                        rule='3x measured floor' if FLOOR_FACTOR * floor >= ROUNDINGS * S.EPS32 else '8 roundings')
    return None if err <= bound else (name, dict(kernel=err, fp32_floor=floor, bound=bound))


def _judge_own(report, name, got, r64, r32, unit=0.0):
    """the floor of this very input set (compositing and the positional encodings: one input set per shape, thousands of elements each)"""
    return _judge(report, name, got, (r64, r32, unit), _row_err(r32, r64, unit))


def _judge_all(report, gots, refs, floors):
    return [_judge(report, k, g, refs[k], floors[k]) for k, g in gots.items()]


def _settle(test_id, report, fails):
    parity_report(test_id, **report)
    fails = [f for f in fails if f]
    assert not fails, fails


def _col4(v):
    """[n] or [n,k<=4] -> raw head layout [n,4] (the unused columns hold junk the kernels must ignore)"""
    v = v.reshape(v.shape[0], -1)
    out = torch.full((v.shape[0], 4), 77.0)
    out[:, :v.shape[1]] = v
    return out


# ---- 1. nero_sdf_alpha_fwd / nero_sdf_alpha_bwd ------------------------------------------------------------------------------------
COMBOS = ((True, True), (False, True), (True, False), (False, False))            # (d_gerr given, d_geo given)


def _alpha_cots(n):
    g = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, 8, generator=g)


@functools.lru_cache(maxsize=None)
def _refs_alpha(n, R, T):
    a = S.alpha_inputs(n, R, T)
    d_alpha, d_gerr, d_geo = _alpha_cots(n)
    out = {}
    for an in ANNEALS:
        f, b = {}, {}
        for dt in (F64, F32):
            c = lambda k: a[k].to(dt)
            f[dt] = S.sdf_alpha(c('sdf4')[:, 0], c('grad'), c('x4')[:, 3], c('d'), a['ray'], S.inv_s_of(a['variance'], dt).expand(n), an)[:3]
            for ug, uo in COMBOS:
                b[dt, ug, uo] = S.sdf_alpha_bwd(a['sdf4'][:, 0], a['grad'], a['x4'][:, 3], a['d'], a['ray'], S.inv_s_of(a['variance'], dt), an,
                                                d_alpha, d_gerr if ug else None, d_geo if uo else None, dtype=dt)
        for i, nm in enumerate(('alpha', 'geo', 'gerr')):
            out[f'{nm}@{an}'] = (f[F64][i], f[F32][i], 1.0 if nm == 'gerr' else 0.0)
        sizes = S.sdf_alpha_term_sizes(a['sdf4'][:, 0], a['grad'], a['x4'][:, 3], a['d'], a['ray'], S.inv_s_of(a['variance'], F64).expand(n), an, d_alpha)
        for ug, uo in COMBOS:
            for i, nm in enumerate(('d_sdf', 'd_grad', 'dinv')):
                out[f'{nm}@{an},gerr={int(ug)},geo={int(uo)}'] = (b[F64, ug, uo][i], b[F32, ug, uo][i], sizes[i])
    return out


@pytest.mark.parametrize('n,R,T', S.PER_SAMPLE)
def test_sdf_alpha_fwd_bwd(n, R, T):
    L = _lib()
    a = S.alpha_inputs(n, R, T)
    d_alpha, d_gerr, d_geo = _alpha_cots(n)
    dev = {k: _cu(a[k]) for k in ('sdf4', 'grad', 'x4', 'idx', 'd', 'variance')}
    gots = {}
    for an in ANNEALS:
        alpha, geo, gerr = _out(n), _out(n, 8), _out(n)
        L.check(L.lib.nero_sdf_alpha_fwd(_p(dev['sdf4']), _p(dev['grad']), _p(dev['x4']), _p(dev['idx']), _p(dev['d']), T, _p(dev['variance']),
                                         C.c_float(an), n, _p(alpha), _p(geo), _p(gerr), L.stream_ptr()))
        gots[f'alpha@{an}'], gots[f'geo@{an}'], gots[f'gerr@{an}'] = _take(alpha, n), _take(geo, n), _take(gerr, n)
        assert bool(((gots[f'alpha@{an}'] >= 0) & (gots[f'alpha@{an}'] <= 1)).all())
        for ug, uo in COMBOS:
            d_sdf4, d_grad, dinv = _out(n, 4, pad=True), _out(n, 3), _out(n, pad=True)
            L.check(L.lib.nero_sdf_alpha_bwd(_p(dev['sdf4']), _p(dev['grad']), _p(dev['x4']), _p(dev['idx']), _p(dev['d']), T, _p(dev['variance']),
                                             C.c_float(an), n, _p(_cu(d_alpha)), _p(_cu(d_gerr) if ug else None),
                                             _p(_cu(d_geo) if uo else None), _p(d_sdf4), _p(d_grad), _p(dinv), L.stream_ptr()))
            gs4, gg, gi = _take(d_sdf4, n, pad=True), _take(d_grad, n), _take(dinv, n, pad=True)
            assert bool((gs4[:, 1:] == 0).all())
            tag = f'@{an},gerr={int(ug)},geo={int(uo)}'
            gots['d_sdf' + tag], gots['d_grad' + tag], gots['dinv' + tag] = gs4[:, 0], gg, gi
    report = {}
    _settle(f'shade_kernels::sdf_alpha[n={n},T={T}]', report, _judge_all(report, gots, _refs_alpha(n, R, T), _floors(_refs_alpha)))


# ---- 2. nero_shade_encode / nero_shade_encode_bwd ---------------------------------------------------------------------------------
def _shade_encode(s, n, sphere):
    L = _lib()
    ldd = 144 if sphere else 72
    mat, Xd, Xs, Xi, Xo = _out(n, 8), _out(n, ldd, pad=True), _out(n, ldd, pad=True), _out(n, 128, pad=True), _out(n, 96, pad=True)
    L.check(L.lib.nero_shade_encode(_p(_cu(s['x4'])), _p(_cu(s['geo'])), _p(_cu(s['m_raw'])), _p(_cu(s['r_raw'])), _p(_cu(s['a_raw'])), n,
                                    _p(mat), _p(Xd), _p(Xs), _p(Xi), _p(Xo), int(sphere), L.stream_ptr()))
    return _take(mat, n), _take(Xd, n, pad=True), _take(Xs, n, pad=True), _take(Xi, n, pad=True), _take(Xo, n, pad=True)


@functools.lru_cache(maxsize=None)
def _refs_encode(n, R, T, sphere):
    s = S.shading_inputs(n, R, T)
    r = {}
    for dt in (F64, F32):
        c = lambda k: s[k].to(dt)
        m = S.materials(c('m_raw'), c('r_raw'), c('a_raw'))
        r[dt] = (m,) + S.shade_encode(c('p'), c('geo')[:, :3], c('geo')[:, 4:7], m[:, 1:2], bool(sphere))[:4]
    return {nm: (r[F64][i], r[F32][i], 0.0) for i, nm in enumerate(('mat', 'Xd', 'Xs', 'Xi', 'Xo'))}


@pytest.mark.parametrize('sphere', [0, 1])
@pytest.mark.parametrize('n,R,T', S.PER_SAMPLE)
def test_shade_encode_fwd(n, R, T, sphere):
    s = S.shading_inputs(n, R, T)
    mat, Xd, Xs, Xi, Xo = _shade_encode(s, n, sphere)
    assert torch.equal(Xi[:, 51:123], Xs[:, :72])                       # the IDE(refl, rough) block, bit for bit
    assert torch.equal(Xi[:, :51], Xo[:, :51]) and bool((Xi[:, 123:] == 0).all()) and bool((Xo[:, 90:] == 0).all())
    assert bool((mat[:, 5:] == 0).all())
    report = {}
    _settle(f'shade_kernels::shade_encode[n={n},sphere={sphere}]', report,
            _judge_all(report, dict(mat=mat, Xd=Xd, Xs=Xs, Xi=Xi, Xo=Xo), _refs_encode(n, R, T, sphere), _floors(_refs_encode, (sphere,))))


@functools.lru_cache(maxsize=None)
def _refs_encode_bwd(n, R, T, sphere):
    s = S.shading_inputs(n, R, T)
    ldd = 144 if sphere else 72
    out = {}
    for ue in (False, True):
        r = {dt: S.shade_encode_bwd(s['p'], s['geo'], s['mat'], s['dXd'][:, :ldd], s['dXs'][:, :ldd], s['dXi'], s['dmat'], s['extra'] if ue else None,
                                    bool(sphere), dtype=dt) for dt in (F64, F32)}
        split = lambda t: (t[0][:, :3], t[0][:, 4:7], t[1], t[2], t[3])
        for nm, r64, r32 in zip(('d_nhat', 'd_refl', 'dm_raw', 'dr_raw', 'da_raw'), split(r[F64]), split(r[F32])):
            out[f'{nm},extra={int(ue)}'] = (r64, r32, 0.0)
    return out


@pytest.mark.parametrize('sphere', [0, 1])
@pytest.mark.parametrize('n,R,T', S.PER_SAMPLE)
def test_shade_encode_bwd(n, R, T, sphere):
    L = _lib()
    s = S.shading_inputs(n, R, T)
    ldd = 144 if sphere else 72
    dXd, dXs = s['dXd'][:, :ldd].contiguous(), s['dXs'][:, :ldd].contiguous()
    gots = {}
    for ue in (False, True):
        d_geo, dm, dr, da = _out(n, 8, pad=True), _out(n, 4, pad=True), _out(n, 4, pad=True), _out(n, 4, pad=True)
        L.check(L.lib.nero_shade_encode_bwd(_p(_cu(s['geo'])), _p(_cu(s['mat'])), _p(_cu(dXd)), _p(_cu(dXs)), _p(_cu(s['dXi'])), _p(_cu(s['dmat'])), n,
                                            _p(d_geo), _p(dm), _p(dr), _p(da), _p(_cu(s['extra']) if ue else None), _p(_cu(s['x4'])),
                                            int(sphere), L.stream_ptr()))
        g_geo, g_m, g_r, g_a = [_take(t, n, pad=True) for t in (d_geo, dm, dr, da)]
        assert torch.equal(g_geo[:, 3], s['dmat'][:, 5]) and bool((g_geo[:, 7] == 0).all())         # d_NoV is a copy
        assert bool((g_m[:, 1:] == 0).all()) and bool((g_r[:, 1:] == 0).all()) and bool((g_a[:, 3] == 0).all())
        for nm, gt in zip(('d_nhat', 'd_refl', 'dm_raw', 'dr_raw', 'da_raw'), (g_geo[:, :3], g_geo[:, 4:7], g_m[:, 0], g_r[:, 0], g_a[:, :3])):
            gots[f'{nm},extra={int(ue)}'] = gt
    report = {}
    _settle(f'shade_kernels::shade_encode_bwd[n={n},sphere={sphere}]', report,
            _judge_all(report, gots, _refs_encode_bwd(n, R, T, sphere), _floors(_refs_encode_bwd, (sphere,))))


# ---- 3. nero_human_encode / nero_human_encode_bwd -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs_human(n, R, T):
    s = S.shading_inputs(n, R, T)
    pp = s['poses'][s['ray']]
    rf, rb = {}, {}
    for dt in (F64, F32):
        c = lambda k: s[k].to(dt)
        rf[dt] = S.human_encode(c('p'), c('geo')[:, 4:7], c('mat')[:, 1:2], pp.to(dt))[:2]
        rb[dt] = S.human_encode_bwd(s['p'], s['geo'], s['mat'], pp, s['dXh'], dtype=dt)
    return dict(Xh=(rf[F64][0], rf[F32][0], 0.0), extra=(rb[F64], rb[F32], 0.0), hmask=(rf[F64][1], rf[F32][1], 0.0))


@pytest.mark.parametrize('n,R,T', S.PER_SAMPLE)
def test_human_encode_fwd_bwd(n, R, T):
    L = _lib()
    s = S.shading_inputs(n, R, T)
    dev = [_cu(s[k]) for k in ('x4', 'geo', 'mat', 'idx')]
    poses = _cu(s['poses'])
    Xh, hmask, extra = _out(n, 24, pad=True), _out(n, pad=True), _out(n, 4)
    L.check(L.lib.nero_human_encode(*[_p(t) for t in dev], T, _p(poses), n, _p(Xh), _p(hmask), L.stream_ptr()))
    L.check(L.lib.nero_human_encode_bwd(*[_p(t) for t in dev], T, _p(poses), n, _p(_cu(s['dXh'])), _p(extra), L.stream_ptr()))
    gX, gh, ge = _take(Xh, n, pad=True), _take(hmask, n, pad=True), _take(extra, n)
    refs = _refs_human(n, R, T)
    assert torch.equal(gh.double(), refs['hmask'][0])                   # the hit mask: exact
    miss = gh == 0
    assert bool((ge[miss] == 0).all()) and bool((gX[miss, :12] == 0).all())          # no hit: sin(0) rows, no gradient
    report = {'rows': dict(hit=int((~miss).sum()), miss=int(miss.sum()))}
    _settle(f'shade_kernels::human_encode[n={n},T={T}]', report, _judge_all(report, dict(Xh=gX, extra=ge), refs, _floors(_refs_human)))


# ---- 4. nero_shade_combine_fwd / nero_shade_combine_bwd / nero_shade_inter_results --------------------------------------------------
REC = (('specular_albedo', 0, 3), ('specular_ref', 3, 6), ('specular_light', 6, 9), ('specular_color', 9, 12), ('diffuse_albedo', 12, 15),
       ('diffuse_light', 15, 18), ('diffuse_color', 18, 21), ('indirect_light', 24, 27), ('human_light', 27, 30))
DMAT = ('d_metallic', 'd_rough', 'd_albedo0', 'd_albedo1', 'd_albedo2', 'd_NoV')


@functools.lru_cache(maxsize=None)
def _refs_combine(n, R, T, human):
    s = S.shading_inputs(n, R, T)
    lut = ref_fg_lut()
    heads = [s[k] for k in ('Ld', 'Ls', 'Li', 'Lo')]
    Lh, hm = (s['Lh'], s['hmask']) if human else (None, None)
    rf, ri, out = {}, {}, {}
    for dt in (F64, F32):
        c = lambda t: None if t is None else t.to(dt)
        args = (c(s['geo'][:, 3]), c(s['mat'])) + tuple(c(h) for h in heads) + (lut, s['exp_max'], c(Lh), c(hm))
        rf[dt], ri[dt] = S.combine_fwd(*args)[:2], S.inter_results(*args)
    out['color'], out['occ_prob'] = (rf[F64][0], rf[F32][0], 0.0), (rf[F64][1], rf[F32][1], 0.0)
    for nm, c0, c1 in REC:
        out['rec.' + nm] = (ri[F64][:, c0:c1], ri[F32][:, c0:c1], 0.0)
    for uo in (False, True):
        r = {dt: S.combine_bwd(s['geo'][:, 3], s['mat'], *heads, lut, s['exp_max'], s['d_color'], s['d_occ'] if uo else None, Lh, hm, dtype=dt)
             for dt in (F64, F32)}
        for i, nm in enumerate(['dLd', 'dLs', 'dLi', 'dLo', 'dmat'] + (['dLh'] if human else [])):
            w = {'dLo': 1, 'dmat': 6, 'dLh': 4}.get(nm, 3)
            out[f'{nm},d_occ={int(uo)}'] = (r[F64][i][:, :w], r[F32][i][:, :w], 0.0)
        lut_size = S.combine_bwd(s['geo'][:, 3], s['mat'], *heads, lut, s['exp_max'], s['d_color'], None, Lh, hm, want_lut_size=True)
        for j, nm in enumerate(DMAT):                                    # per column too: a row maximum would hide d_NoV behind d_albedo
            out[f'dmat.{nm},d_occ={int(uo)}'] = (r[F64][4][:, j], r[F32][4][:, j], lut_size if nm in ('d_rough', 'd_NoV') else 0.0)
    return out


@pytest.mark.parametrize('human', [0, 1])
@pytest.mark.parametrize('n,R,T', S.PER_SAMPLE)
def test_shade_combine_and_inter_results(n, R, T, human):
    L = _lib()
    s = S.shading_inputs(n, R, T)
    heads = [s[k] for k in ('Ld', 'Ls', 'Li', 'Lo')]
    dev = [_cu(s['geo']), _cu(s['mat'])] + [_cu(h) for h in heads] + [_cu(ref_fg_lut())]
    Lh, hm = (_cu(s['Lh']), _cu(s['hmask'])) if human else (None, None)
    ex = C.c_float(s['exp_max'])
    color, occ, rec = _out(n, 3), _out(n), _out(n, 32)
    L.check(L.lib.nero_shade_combine_fwd(*[_p(t) for t in dev], ex, n, _p(color), _p(occ), _p(Lh), _p(hm), L.stream_ptr()))
    L.check(L.lib.nero_shade_inter_results(*[_p(t) for t in dev], ex, n, _p(Lh), _p(hm), _p(rec), L.stream_ptr()))
    gc, go, gr = _take(color, n), _take(occ, n), _take(rec, n)
    gots = dict(color=gc, occ_prob=go)
    for nm, c0, c1 in REC:
        gots['rec.' + nm] = gr[:, c0:c1]
    # cross-checks without a tolerance: the copies and the occlusion value both calls share
    assert torch.equal(gr[:, 21], s['mat'][:, 0]) and torch.equal(gr[:, 22], s['mat'][:, 1]) and bool((gr[:, 30:] == 0).all())
    assert torch.equal(gr[:, 23], go.clamp(0.0, 1.0))
    assert bool(((gc >= 0) & (gc <= 1)).all())
    if not human:
        assert bool((gr[:, 27:30] == 0).all())
    for uo in (False, True):
        dL = [_out(n, 4, pad=True) for _ in range(4)]
        dmat, dLh = _out(n, 8), (_out(n, 4, pad=True) if human else None)
        L.check(L.lib.nero_shade_combine_bwd(*[_p(t) for t in dev], ex, n, _p(_cu(s['d_color'])), _p(_cu(s['d_occ']) if uo else None),
                                             *[_p(t) for t in dL], _p(dmat), _p(None), _p(Lh), _p(hm), _p(dLh), L.stream_ptr()))
        got = [_take(t, n, pad=True) for t in dL] + [_take(dmat, n)] + ([_take(dLh, n, pad=True)] if human else [])
        assert all(bool((got[i][:, 3] == 0).all()) for i in range(3)) and bool((got[3][:, 1:] == 0).all()) and bool((got[4][:, 6:] == 0).all())
        for i, nm in enumerate(['dLd', 'dLs', 'dLi', 'dLo', 'dmat'] + (['dLh'] if human else [])):
            gots[f'{nm},d_occ={int(uo)}'] = got[i][:, :{'dLo': 1, 'dmat': 6, 'dLh': 4}.get(nm, 3)]
        for j, nm in enumerate(DMAT):
            gots[f'dmat.{nm},d_occ={int(uo)}'] = got[4][:, j]
    report = {}
    _settle(f'shade_kernels::combine[n={n},human={human}]', report,
            _judge_all(report, gots, _refs_combine(n, R, T, human), _floors(_refs_combine, (human,))))


# ---- 5. nero_nerf_head_fwd / nero_nerf_head_bwd ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs_nerf(n, R=0, T=0):
    q = S.nerf_inputs(n)
    f = {dt: S.nerf_head(q['sig4'][:, 0].to(dt), q['rgb4'][:, :3].to(dt), q['dist'].to(dt))[:2] for dt in (F64, F32)}
    b = {dt: S.nerf_head_bwd(q['sig4'][:, 0], q['rgb4'][:, :3], q['dist'], q['d_alpha'], q['d_color'], dtype=dt) for dt in (F64, F32)}
    return dict(alpha=(f[F64][0], f[F32][0], 1.0), color=(f[F64][1], f[F32][1], 0.0), d_sig=(b[F64][0], b[F32][0], 0.0), d_rgb=(b[F64][1], b[F32][1], 0.0))


@pytest.mark.parametrize('n', NS)
def test_nerf_head_fwd_bwd(n):
    L = _lib()
    q = S.nerf_inputs(n)
    dev = [_cu(q['sig4']), _cu(q['rgb4']), _cu(q['dist'])]
    alpha, color, d_sig4, d_rgb4 = _out(n), _out(n, 3), _out(n, 4, pad=True), _out(n, 4, pad=True)
    L.check(L.lib.nero_nerf_head_fwd(*[_p(t) for t in dev], n, _p(alpha), _p(color), L.stream_ptr()))
    L.check(L.lib.nero_nerf_head_bwd(*[_p(t) for t in dev], n, _p(_cu(q['d_alpha'])), _p(_cu(q['d_color'])), _p(d_sig4), _p(d_rgb4), L.stream_ptr()))
    ga, gc, gs, gr = _take(alpha, n), _take(color, n), _take(d_sig4, n, pad=True), _take(d_rgb4, n, pad=True)
    assert bool((gs[:, 1:] == 0).all()) and bool((gr[:, 3] == 0).all())
    if n > 8:
        assert float(ga[7]) == 0.0 and float(gs[7, 0]) == 0.0                 # dist == 0
        assert float(gr[5, 1]) == 0.0 and float(gr[4, 0]) != 0.0              # rgb raw above 5: no gradient; exactly 5: clamp passes it
    report = {}
    _settle(f'shade_kernels::nerf_head[n={n}]', report,
            _judge_all(report, dict(alpha=ga, color=gc, d_sig=gs[:, 0], d_rgb=gr[:, :3]), _refs_nerf(n), _floors(_refs_nerf)))


# ---- 6. nero_scatter_samples / nero_gather_sample_grads ------------------------------------------------------------------------------
@pytest.mark.parametrize('n,R,T', [(1, 3, 1), (65, 5, 160), (129, 7, 40), (200, 4, 63)])
def test_scatter_and_gather_are_exact(n, R, T):
    L = _lib()
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(R * T, generator=g)
    inner, outer = torch.sort(perm[:n])[0].int(), torch.sort(perm[n:])[0].int()
    aRT, cRT = _f(R * T + GUARD), _f(R * T + GUARD, 3)
    a_i, c_i = torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    L.check(L.lib.nero_scatter_samples(_p(_cu(a_i)), _p(_cu(c_i)), _p(_cu(inner)), n, _p(aRT), _p(cRT), L.stream_ptr()))
    ra, rc = S.scatter(a_i, c_i, inner, R * T + GUARD, SENT)
    assert torch.equal(aRT.cpu(), ra) and torch.equal(cRT.cpu(), rc)         # untouched slots keep the sentinel
    m = outer.numel()
    a_o, c_o = torch.randn(m, generator=g), torch.randn(m, 3, generator=g)
    L.check(L.lib.nero_scatter_samples(_p(_cu(a_o)), _p(_cu(c_o)), _p(_cu(outer)), m, _p(aRT), _p(cRT), L.stream_ptr()))
    ra[outer.long()], rc[outer.long()] = a_o, c_o
    assert torch.equal(aRT.cpu(), ra) and torch.equal(cRT.cpu(), rc)
    assert not bool((aRT[:R * T] == SENT).any()) and _untouched(aRT[R * T:]) and _untouched(cRT[R * T:])   # together: R*T exactly once
    d_a, d_c = _out(n), _out(n, 3)
    L.check(L.lib.nero_gather_sample_grads(_p(aRT), _p(cRT), _p(_cu(inner)), n, _p(d_a), _p(d_c), L.stream_ptr()))
    assert torch.equal(_take(d_a, n), ra[inner.long()]) and torch.equal(_take(d_c, n), rc[inner.long()])


# ---- 7. nero_composite_fwd / nero_composite_bwd ----------------------------------------------------------------------------------------
def _composite(q, R, T):
    L = _lib()
    a, c = _cu(q['alpha'][:R]), _cu(q['color'][:R])
    w, rgb, d_a, d_c = _out(R, T), _out(R, 3), _out(R, T), _out(R, T, 3)
    L.check(L.lib.nero_composite_fwd(_p(a), _p(c), R, T, _p(w), _p(rgb), L.stream_ptr()))
    L.check(L.lib.nero_composite_bwd(_p(a), _p(c), _p(w), _p(_cu(q['d_rgb'][:R])), R, T, _p(d_a), _p(d_c), L.stream_ptr()))
    return [_take(t, R) for t in (w, rgb, d_a, d_c)]


def _composite_refs(q):
    out = {'size': S.composite_bwd_term_sizes(q['alpha'], q['color'], q['d_rgb'])}
    for dt in (F64, F32):
        w, rgb, _ = S.composite(q['alpha'].to(dt), q['color'].to(dt))
        out[dt] = (w, rgb) + tuple(S.composite_bwd(q['alpha'], q['color'], q['d_rgb'], dtype=dt))
    return out


@pytest.mark.parametrize('T', S.COMPOSITE_WAVE_T + S.COMPOSITE_THREAD_T)
def test_composite_fwd_bwd(T):
    Rs = S.WAVE_R if T <= 192 else S.THREAD_R
    q = S.composite_inputs(max(Rs), T)
    refs = _composite_refs(q)
    report, fails = {}, []
    full = None
    for R in sorted(Rs, reverse=True):
        got = _composite(q, R, T)
        if full is None:
            full = got
            for i, nm in enumerate(('weights', 'rgb', 'd_alpha', 'd_color')):
                # weights / d_alpha / d_color element by element: an opaque sample's neighbours are the point
                el = (lambda t: t.reshape(-1)) if nm != 'rgb' else (lambda t: t)
                fails.append(_judge_own(report, nm, el(got[i]), el(refs[F64][i]), el(refs[F32][i]), el(refs['size']) if nm == 'd_alpha' else 0.0))
                fails.append(_judge_own(report, nm + '.opaque_ray', el(got[i][:1]), el(refs[F64][i][:1]), el(refs[F32][i][:1]),
                                        el(refs['size'][:1]) if nm == 'd_alpha' else 0.0))
        else:
            assert all(torch.equal(g_, f_[:R]) for g_, f_ in zip(got, full)), R          # a ray does not depend on R
    _settle(f'shade_kernels::composite[T={T}]', report, fails)


def test_composite_wave_and_thread_paths_agree_on_shared_columns():
    """T = 192 (one wavefront per ray) and T = 193 (one thread per ray) on identical rays, the 193rd sample transparent (alpha = 0: it takes no
    weight and hands no gradient to the samples before it): both paths against ONE reference on the shared 192 columns"""
    R = 5
    q = S.composite_inputs(R, 192)
    q193 = dict(alpha=torch.cat([q['alpha'], torch.zeros(R, 1)], 1), color=torch.cat([q['color'], torch.rand(R, 1, 3)], 1), d_rgb=q['d_rgb'])
    refs = _composite_refs(q)
    wave, thread = _composite(q, R, 192), _composite(q193, R, 193)
    report, fails = {}, []
    for i, nm in enumerate(('weights', 'rgb', 'd_alpha', 'd_color')):
        cut = (lambda t: t) if nm == 'rgb' else (lambda t: t[:, :192].reshape(-1))
        el = (lambda t: t) if nm == 'rgb' else (lambda t: t.reshape(-1))
        fails.append(_judge_own(report, nm + '.wave', el(wave[i]), el(refs[F64][i]), el(refs[F32][i]), el(refs['size']) if nm == 'd_alpha' else 0.0))
        fails.append(_judge_own(report, nm + '.thread', cut(thread[i]), el(refs[F64][i]), el(refs[F32][i]), el(refs['size']) if nm == 'd_alpha' else 0.0))
    assert bool((thread[0][:, 192] == 0).all())
    _settle('shade_kernels::composite_wave_vs_thread', report, fails)


# ---- 8. nero_encode_pe / nero_pe_vjp / nero_pe_jvp -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200, 257])
def test_pe_calls(n):
    L = _lib()
    g = torch.Generator().manual_seed(n)
    report, fails = {}, []
    from oracle import nero_oracle as O
    for n_freq, dim, ldx, ldo in ((0, 3, 3, 3), (6, 3, 4, 40), (8, 3, 5, 56), (10, 4, 4, 88)):        # ldx > dim; ldo == width and > width
        x = torch.randn(n, ldx, generator=g)
        width = dim * (1 + 2 * n_freq)
        out = _out(n, ldo, pad=True)
        L.check(L.lib.nero_encode_pe(_p(_cu(x)), ldx, dim, n_freq, n, _p(out), ldo, L.stream_ptr()))
        got = _take(out, n, pad=True)
        assert torch.equal(got[:, :dim], x[:, :dim]) and bool((got[:, width:] == 0).all())
        fails.append(_judge_own(report, f'encode_pe[L={n_freq},dim={dim}]', got[:, :width], O.pos_enc(x[:, :dim].double(), n_freq), O.pos_enc(x[:, :dim], n_freq)))
    for n_freq in (0, 3, 6):
        nv = 3 * (1 + 2 * n_freq)
        x4, t4 = torch.randn(n, 4, generator=g), torch.randn(n, 5, generator=g)
        e0, e1 = torch.randn(n, 40, generator=g), torch.randn(n, 48, generator=g)
        for use_e1 in (True, False):
            out = _out(n, 4)
            L.check(L.lib.nero_pe_vjp(_p(_cu(x4)), 4, _p(_cu(e0)), 40, _p(_cu(e1) if use_e1 else None), 48, n_freq, n, _p(out), 4, L.stream_ptr()))
            got = _take(out, n)
            assert _untouched(got[:, 3])                                     # the pitch column is left alone
            e = e0[:, :nv] + (e1[:, :nv] if use_e1 else 0)
            # (the kernel adds e0 + e1 in float32 first: the references get that sum, its own input)
            fails.append(_judge_own(report, f'pe_vjp[L={n_freq},e1={int(use_e1)}]', got[:, :3], S.pe_vjp(x4[:, :3], e, n_freq), S.pe_vjp(x4[:, :3], e, n_freq, dtype=F32)))
        for ldo in sorted({nv, 40}):
            out = _out(n, ldo, pad=True)
            L.check(L.lib.nero_pe_jvp(_p(_cu(x4)), 4, _p(_cu(t4)), 5, n_freq, n, _p(out), ldo, L.stream_ptr()))
            got = _take(out, n, pad=True)
            assert bool((got[:, nv:] == 0).all()) and torch.equal(got[:, :3], t4[:, :3])
            fails.append(_judge_own(report, f'pe_jvp[L={n_freq},ldo={ldo}]', got[:, :nv], S.pe_jvp(x4[:, :3], t4[:, :3], n_freq), S.pe_jvp(x4[:, :3], t4[:, :3], n_freq, dtype=F32)))
    _settle(f'shade_kernels::pe[n={n}]', report, fails)


# ---- 9. argument checks: NERO_ERR_ARG before any launch, nothing written -----------------------------------------------------------
def test_bad_arguments_are_refused_before_a_launch():
    L = _lib()
    n, R, T = 5, 3, 4
    st = L.stream_ptr()
    bufs = [_f(64 * 160) for _ in range(24)]
    idx = _cu(torch.zeros(64, dtype=torch.int32))
    b = [_p(t) for t in bufs]
    i, NUL, f0 = _p(idx), _p(None), C.c_float(0.5)
    lib = L.lib
    calls = {
        'nero_sdf_alpha_fwd': lambda a, n_=n, T_=T: lib.nero_sdf_alpha_fwd(a[0], a[1], a[2], i, a[3], T_, a[4], f0, n_, a[5], a[6], a[7], st),
        'nero_sdf_alpha_bwd': lambda a, n_=n, T_=T: lib.nero_sdf_alpha_bwd(a[0], a[1], a[2], i, a[3], T_, a[4], f0, n_, a[5], NUL, NUL, a[6], a[7], a[8], st),
        'nero_shade_encode': lambda a, n_=n, T_=T: lib.nero_shade_encode(a[0], a[1], a[2], a[3], a[4], n_, a[5], a[6], a[7], a[8], a[9], 0, st),
        'nero_shade_combine_fwd': lambda a, n_=n, T_=T: lib.nero_shade_combine_fwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], f0, n_, a[7], a[8], NUL, NUL, st),
        'nero_shade_inter_results': lambda a, n_=n, T_=T: lib.nero_shade_inter_results(a[0], a[1], a[2], a[3], a[4], a[5], a[6], f0, n_, NUL, NUL, a[7], st),
        'nero_shade_combine_bwd': lambda a, n_=n, T_=T: lib.nero_shade_combine_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6], f0, n_, a[7], NUL, a[8], a[9],
                                                                                   a[10], a[11], a[12], NUL, NUL, NUL, NUL, st),
        'nero_shade_encode_bwd': lambda a, n_=n, T_=T: lib.nero_shade_encode_bwd(a[0], a[1], a[2], a[3], a[4], a[5], n_, a[6], a[7], a[8], a[9], NUL, NUL, 0, st),
        'nero_human_encode': lambda a, n_=n, T_=T: lib.nero_human_encode(a[0], a[1], a[2], i, T_, a[3], n_, a[4], a[5], st),
        'nero_human_encode_bwd': lambda a, n_=n, T_=T: lib.nero_human_encode_bwd(a[0], a[1], a[2], i, T_, a[3], n_, a[4], a[5], st),
        'nero_nerf_head_fwd': lambda a, n_=n, T_=T: lib.nero_nerf_head_fwd(a[0], a[1], a[2], n_, a[3], a[4], st),
        'nero_nerf_head_bwd': lambda a, n_=n, T_=T: lib.nero_nerf_head_bwd(a[0], a[1], a[2], n_, a[3], a[4], a[5], a[6], st),
        'nero_scatter_samples': lambda a, n_=n, T_=T: lib.nero_scatter_samples(a[0], a[1], i, n_, a[2], a[3], st),
        'nero_gather_sample_grads': lambda a, n_=n, T_=T: lib.nero_gather_sample_grads(a[0], a[1], i, n_, a[2], a[3], st),
        'nero_composite_fwd': lambda a, n_=R, T_=T: lib.nero_composite_fwd(a[0], a[1], n_, T_, a[2], a[3], st),
        'nero_composite_bwd': lambda a, n_=R, T_=T: lib.nero_composite_bwd(a[0], a[1], a[2], a[3], n_, T_, a[4], a[5], st),
        'nero_pe_vjp': lambda a, n_=n, T_=T: lib.nero_pe_vjp(a[0], 4, a[1], 40, NUL, 0, 6, n_, a[2], 4, st),
        'nero_pe_jvp': lambda a, n_=n, T_=T: lib.nero_pe_jvp(a[0], 4, a[1], 4, 6, n_, a[2], 40, st),
        'nero_encode_pe': lambda a, n_=n, T_=T: lib.nero_encode_pe(a[0], 4, 3, 6, n_, a[1], 40, st),
    }
    n_ptr = dict(nero_sdf_alpha_fwd=8, nero_sdf_alpha_bwd=9, nero_shade_encode=10, nero_shade_combine_fwd=9, nero_shade_inter_results=8,
                 nero_shade_combine_bwd=13, nero_shade_encode_bwd=10, nero_human_encode=6, nero_human_encode_bwd=6, nero_nerf_head_fwd=5,
                 nero_nerf_head_bwd=7, nero_scatter_samples=4, nero_gather_sample_grads=4, nero_composite_fwd=4, nero_composite_bwd=6,
                 nero_pe_vjp=3, nero_pe_jvp=3, nero_encode_pe=2)
    uses_T = ('nero_sdf_alpha_fwd', 'nero_sdf_alpha_bwd', 'nero_human_encode', 'nero_human_encode_bwd', 'nero_composite_fwd', 'nero_composite_bwd')
    refused = 0
    for name, call in calls.items():
        for k in range(n_ptr[name]):                                          # every required pointer in turn
            a = list(b)
            a[k] = NUL
            assert call(a) == -1, (name, 'NULL pointer', k)
            refused += 1
        assert call(b, n_=-1) == -1, (name, 'negative count')
        assert call(b, n_=0) == 0, (name, 'empty call')
        refused += 1
        if name in uses_T:
            assert call(b, T_=0) == -1 and call(b, T_=-3) == -1, (name, 'T < 1')
            refused += 2
    # the sample index list, and the encodings' own ranges
    for name in ('nero_sdf_alpha_fwd', 'nero_sdf_alpha_bwd', 'nero_human_encode', 'nero_human_encode_bwd', 'nero_scatter_samples', 'nero_gather_sample_grads'):
        i = NUL
        assert calls[name](b) == -1, (name, 'NULL idx')
        refused += 1
    i = _p(idx)
    x, o = b[0], b[1]
    assert lib.nero_encode_pe(x, 4, 3, -1, n, o, 40, st) == -1 and lib.nero_encode_pe(x, 4, 5, 2, n, o, 40, st) == -1
    assert lib.nero_encode_pe(x, 4, 3, 7, n, o, 40, st) == -1                                         # 3 (1 + 14) > ldo
    assert lib.nero_pe_vjp(x, 4, b[2], 40, NUL, 0, 7, n, o, 4, st) == -1 and lib.nero_pe_vjp(x, 4, b[2], 40, NUL, 0, -1, n, o, 4, st) == -1
    assert lib.nero_pe_jvp(x, 4, b[2], 4, 7, n, o, 48, st) == -1 and lib.nero_pe_jvp(x, 4, b[2], 4, 6, n, o, 38, st) == -1
    assert lib.nero_pe_jvp(x, 4, b[2], 4, 2, n, o, 41, st) == -1                                      # ldo > 40
    refused += 8
    # human light: Lh and hmask come together, dLh exactly with Lh
    for Lh, hm, dLh in ((b[13], NUL, NUL), (NUL, b[14], NUL), (b[13], b[14], NUL), (NUL, NUL, b[15])):
        assert lib.nero_shade_combine_bwd(b[0], b[1], b[2], b[3], b[4], b[5], b[6], f0, n, b[7], NUL, b[8], b[9], b[10], b[11], b[12], NUL, Lh, hm, dLh, st) == -1
        refused += 1
    for Lh, hm in ((b[13], NUL), (NUL, b[14])):
        assert lib.nero_shade_combine_fwd(b[0], b[1], b[2], b[3], b[4], b[5], b[6], f0, n, b[7], b[8], Lh, hm, st) == -1
        assert lib.nero_shade_inter_results(b[0], b[1], b[2], b[3], b[4], b[5], b[6], f0, n, Lh, hm, b[7], st) == -1
        refused += 2
    assert lib.nero_shade_encode_bwd(b[0], b[1], b[2], b[3], b[4], b[5], n, b[6], b[7], b[8], b[9], NUL, NUL, 1, st) == -1      # sphere_direction needs x4
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in bufs), 'a refused call wrote to a buffer'
    assert b'bad argument' in lib.nero_last_error() or b'needs' in lib.nero_last_error()
    parity_report('shade_kernels::bad_arguments', refused_calls=refused)
