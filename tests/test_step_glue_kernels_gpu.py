"""GPU tier: every entry point of nero_amd/csrc/step_glue.hip called directly through the C ABI against tests/glue_ref.py (pinned by
tests/test_glue_ref_cpu.py), at the smallest shapes that cross each boundary of the kernels: the 256-thread blocks, the 1024-sample scan
blocks, the 256 scan blocks one pass of occ_scan_kernel covers (n = 262144 / 262145 / 263169: 256, 257 and 258 blocks), the 256 block
partials one strided pass of loss_final_kernel covers (257 and 258 blocks), the 1024-thread stride of occ_l1_kernel and the 4096-slot
in-LDS sort of the kept indices.

Compared against: the float64 restatement evaluated on the kernel's own float32 inputs.  Integers, copies, zeros, refusals and guards are
exact.  Element-wise float outputs, PER ROW: |got - ref64| / max(|ref64| of the row, unit) <= max(3 x floor, 8 x 2^-24), the floor being the
worst row of the float32 restatement against float64 over all cases of the entry point's family (CPU).  Loss terms: the bound derived from
the fixed summation order, (22 + ceil(nb / 256)) x 2^-24 relative (tests/glue_ref.py), two roundings more for the total.  No bound is
computed from a kernel's output, no case and no row is left out, every measured figure goes to parity_report.  Every output is filled with
a sentinel and has guard rows (the select workspace: 256 guard bytes) behind it that must come back untouched; every refused call returns
before any launch (step_glue.hip checks its arguments first) and must leave every buffer as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_ref as G
from tests.helpers import parity_report

pytestmark = pytest.mark.gpu
P = C.c_void_p
SENT, ISENT, BSENT = -12345.0, -7, 0xA5
GUARD, WS_GUARD = 3, 256
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
F32, F64 = G.F32, G.F64


def _lib():
    from nero_amd import _lib as L
    return L


def _p(t, offset=0):
    return P(None if t is None else t.data_ptr() + offset)


_ALIVE = []


def _cu(t):
    """device copy of an input, kept alive until the test ends (the calls below take raw pointers)"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    _ALIVE.append(t.contiguous().cuda())
    return _ALIVE[-1]


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def _f(*shape):
    _ALIVE.append(torch.full(shape, SENT, dtype=F32, device='cuda'))
    return _ALIVE[-1]


def _i(*shape):
    _ALIVE.append(torch.full(shape, ISENT, dtype=torch.int32, device='cuda'))
    return _ALIVE[-1]


def _untouched(t):
    return bool((t == (SENT if t.dtype == F32 else ISENT if t.dtype == torch.int32 else BSENT)).all())


def _take(buf, n):
    """the n live rows (cpu); the guard rows behind must be untouched"""
    assert buf.shape[0] == n + GUARD and _untouched(buf[n:]), 'guard rows written'
    return buf[:n].cpu()


def _second_stream(fn):
    """fn() with a fresh stream current, after everything queued so far has finished"""
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = fn()
    s.synchronize()
    return out


def _judge(report, name, got, r64, r32, floor, unit=0.0):
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert bool(torch.isfinite(got).all()), name
    err, own, bound = G.row_err(got, r64, unit), G.row_err(r32, r64, unit), G.bound_of(floor)
    report[name] = dict(shape=list(got.shape), fp32_floor=floor, fp32_floor_this_case=own, kernel=err, bound=bound,
                        rule='3x measured floor' if G.FLOOR_FACTOR * floor >= G.ROUNDINGS * G.EPS32 else '8 roundings')
    return None if err <= bound else (name, dict(kernel=err, fp32_floor=floor, bound=bound))


def _judge_loss(report, name, got, r64, r32, bound, N):
    """one loss term against its DERIVED bound; an absent term (bound 0) is exactly 0.0"""
    got, r64, r32 = float(got), float(r64), float(r32)
    assert np.isfinite(got), name
    err = G.rel(got, r64)
    report[name] = dict(terms=N, kernel=err, fp32_restatement=G.rel(r32, r64), bound=bound, rule='derived from the summation order' if bound else 'exactly zero')
    ok = (got == 0.0 and r64 == 0.0) if bound == 0.0 else err <= bound
    return None if ok else (name, dict(kernel=got, float64=r64, err=err, bound=bound))


def _settle(test_id, report, fails):
    parity_report(test_id, **report)
    fails = [f for f in fails if f]
    assert not fails, fails


# ---- 1. nero_near_far_sphere --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', G.NEAR_FAR_R)
def test_near_far(R):
    """near_far_kernel: `if (r >= R) return` across the 256-thread block (R = 255, 256, 257, 1000), `mid = 0.5f * (-b) / a` with a != 1
    (directions scaled by 1e-3 / 1e3), a cancelling `b` (rays perpendicular to o) and `fmaxf(mid - 1.0f, 1e-3f)` on rays that start inside
    the sphere, where near is exactly the float32 1e-3.  R = 1 runs one ray of every kind."""
    L = _lib()
    floors = G.near_far_floors()
    report, fails = {}, []
    for R_, shift in [c for c in G.near_far_family() if c[0] == R]:
        q = G.near_far_inputs(R_, shift)
        o, d = _cu(q['o']), _cu(q['d'])
        near, far = _f(R + GUARD), _f(R + GUARD)
        L.check(L.lib.nero_near_far_sphere(_p(o), _p(d), R, _p(near), _p(far), L.stream_ptr()))
        gn, gf = _take(near, R), _take(far, R)
        n64, f64, unit = G.near_far(q['o'], q['d'])
        n32, f32, _ = G.near_far(q['o'], q['d'], F32)
        inside = (q['kind'] == G.INSIDE[0]) | (q['kind'] == G.INSIDE[1])
        assert bool((gn[inside] == float(np.float32(1e-3))).all()) and bool((gn >= float(np.float32(1e-3))).all())
        tag = f'[{G.RAY_KINDS[shift]}]' if R == 1 else ''
        fails.append(_judge(report, 'near' + tag, gn, n64, n32, floors['near'], unit))
        fails.append(_judge(report, 'far' + tag, gf, f64, f32, floors['far'], unit))
    _settle(f'step_glue_kernels::near_far[R={R}]', report, fails)


def test_near_far_empty_and_refused():
    """nero_near_far_sphere: `if (R <= 0) return NERO_OK` and the NULL check in front of the launch"""
    L = _lib()
    q = G.near_far_inputs(257, 0)
    o, d, near, far = _cu(q['o']), _cu(q['d']), _f(257 + GUARD), _f(257 + GUARD)
    st = L.stream_ptr()
    assert L.lib.nero_near_far_sphere(_p(o), _p(d), 0, _p(near), _p(far), st) == OK
    assert L.lib.nero_near_far_sphere(_p(None), _p(None), 0, _p(None), _p(None), st) == OK
    for k in range(4):
        a = [_p(o), _p(d), _p(near), _p(far)]
        a[k] = _p(None)
        assert L.lib.nero_near_far_sphere(a[0], a[1], 257, a[2], a[3], st) == ERR_ARG, k
    torch.cuda.synchronize()
    assert _untouched(near) and _untouched(far)
    parity_report('step_glue_kernels::near_far_refusals', refused_calls=4, empty_calls=2)


# ---- 2. nero_occ_select ---------------------------------------------------------------------------------------------------------------
def _select(L, flag, n, keys, cap):
    """one call on the current stream: workspace of exactly nero_occ_select_workspace(n) bytes + 256 guard bytes -> (cand, counts) on the CPU"""
    ws_bytes = L.lib.nero_occ_select_workspace(n)
    ws = torch.full((ws_bytes + WS_GUARD,), BSENT, dtype=torch.uint8, device='cuda')
    cand, counts = _i(cap + GUARD), _i(2 + GUARD)
    _ALIVE.append(ws)
    L.check(L.lib.nero_occ_select(_p(flag), n, _p(keys), cap, _p(cand), _p(counts), _p(ws), ws_bytes, L.stream_ptr()))
    torch.cuda.current_stream().synchronize()
    assert _untouched(ws[ws_bytes:]), 'bytes behind the workspace written'
    return _take(cand, cap).numpy(), _take(counts, 2).tolist(), ws_bytes


@pytest.mark.parametrize('name', sorted(G.SELECT_CASES))
def test_occ_select(name):
    """exact against the header contract.  Aimed at: occ_count_kernel / occ_records_kernel `base + j < n` (n = 1, 1023, 1024, 1025, 4097),
    occ_scan_kernel's `for (b0 = 0; b0 < nb; b0 += LB)` and its carried `run` (256, 257 and 258 scan blocks; candidates only behind block
    255), `counts[0] = run < cap ? run : cap` (total == cap, cap + 1), `flag[base + j]` read as a truth value (bytes 2 and 255),
    occ_records_kernel's key of a non-candidate (+inf, NaN and signed-zero keys of candidates), occ_pick_kernel's `m2` (cap = 1, 2, 3, 100,
    4095, 4096) and its `-1` fill.  Two runs and a run on a second stream give the same bits."""
    L = _lib()
    n, cap = G.SELECT_CASES[name][:2]
    flag, keys = G.select_inputs(name)
    want_cand, want_counts = G.occ_select(flag, keys, cap)
    fd, kd = _cu(flag), _cu(keys)
    runs = [_select(L, fd, n, kd, cap), _select(L, fd, n, kd, cap), _second_stream(lambda: _select(L, fd, n, kd, cap))]
    parity_report(f'step_glue_kernels::occ_select[{name}]', n=n, cap=cap, scan_blocks=-(-n // G.SB), scan_rounds=G.scan_rounds(n),
                  total=want_counts[1], kept=want_counts[0], finite_keys=int(np.isfinite(keys[:want_counts[1]]).sum()),
                  workspace_bytes=runs[0][2], counts=runs[0][1], wrong_slots=int((runs[0][0] != want_cand).sum()))
    for cand, counts, _ in runs:
        assert counts == list(want_counts), (counts, want_counts)
        assert np.array_equal(cand, want_cand), (int((cand != want_cand).sum()), cand[:8].tolist(), want_cand[:8].tolist())


def test_occ_select_refusals():
    """nero_occ_select: the four argument checks in front of the first launch -- `n <= 0 || cap <= 0`, `cap > PICK_MAX`, a NULL pointer,
    `ws_bytes < nero_occ_select_workspace(n)` -- leave cand, counts and the workspace as they were"""
    L = _lib()
    lib = L.lib
    n, cap = 1025, 100
    flag, keys = G.select_inputs('n1025_total_is_cap100_plus1')
    fd, kd = _cu(flag), _cu(keys)
    ws_bytes = lib.nero_occ_select_workspace(n)
    assert ws_bytes > 0 and lib.nero_occ_select_workspace(0) == 0 and lib.nero_occ_select_workspace(-5) == 0
    ws = torch.full((ws_bytes + WS_GUARD,), BSENT, dtype=torch.uint8, device='cuda')
    cand, counts = _i(G.PICK_MAX + 1 + GUARD), _i(2 + GUARD)
    st = L.stream_ptr()
    call = lambda a, n_=n, cap_=cap, wb=ws_bytes: lib.nero_occ_select(a[0], n_, a[1], cap_, a[2], a[3], a[4], wb, st)
    b = [_p(fd), _p(kd), _p(cand), _p(counts), _p(ws)]
    assert call(b, cap_=G.PICK_MAX + 1) == ERR_UNSUPPORTED
    assert call(b, n_=0) == ERR_ARG and call(b, cap_=0) == ERR_ARG and call(b, n_=-1) == ERR_ARG and call(b, cap_=-1) == ERR_ARG
    for k in range(5):
        a = list(b)
        a[k] = _p(None)
        assert call(a) == ERR_ARG, k
    assert call(b, wb=ws_bytes - 1) == ERR_ARG and call(b, wb=0) == ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(cand) and _untouched(counts) and _untouched(ws), 'a refused call wrote to a buffer'
    parity_report('step_glue_kernels::occ_select_refusals', refused_calls=12, workspace_bytes=ws_bytes)


# ---- 3. nero_occ_gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap,variant', G.GATHER_CASES)
def test_occ_gather(cap, variant):
    """occ_gather_kernel: `if (k >= cap) return` (cap = 1, 255, 256, 257), the `i < 0` slot (origin, +z) at the end and in the middle of
    the list, and the strides `x4[4 * i + c]` / `geo[8 * i + 4 + c]`: every element of x4 and geo is a different number"""
    L = _lib()
    q = G.gather_inputs(cap, variant)
    pts, dirs = _f(cap + GUARD, 3), _f(cap + GUARD, 3)
    L.check(L.lib.nero_occ_gather(_p(_cu(q['x4'])), _p(_cu(q['geo'])), _p(_cu(q['cand'])), cap, _p(pts), _p(dirs), L.stream_ptr()))
    want_p, want_d = G.occ_gather(q['x4'], q['geo'], q['cand'])
    assert torch.equal(_take(pts, cap), want_p) and torch.equal(_take(dirs, cap), want_d)
    parity_report(f'step_glue_kernels::occ_gather[cap={cap},{variant}]', cap=cap, unused_slots=int((q['cand'] < 0).sum()))


def test_occ_gather_empty_and_refused():
    """nero_occ_gather: `if (cap <= 0) return NERO_OK` and the NULL check, both in front of the launch"""
    L = _lib()
    q = G.gather_inputs(256, 'holes')
    x4, geo, cand, pts, dirs = _cu(q['x4']), _cu(q['geo']), _cu(q['cand']), _f(256 + GUARD, 3), _f(256 + GUARD, 3)
    st = L.stream_ptr()
    assert L.lib.nero_occ_gather(_p(x4), _p(geo), _p(cand), 0, _p(pts), _p(dirs), st) == OK
    for k in range(5):
        a = [_p(x4), _p(geo), _p(cand), _p(pts), _p(dirs)]
        a[k] = _p(None)
        assert L.lib.nero_occ_gather(a[0], a[1], a[2], 256, a[3], a[4], st) == ERR_ARG, k
    torch.cuda.synchronize()
    assert _untouched(pts) and _untouched(dirs)


# ---- 4. nero_occ_l1 / nero_occ_l1_backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap,kept,n_in', G.L1_CASES)
def test_occ_l1_fwd_bwd(cap, kept, n_in):
    """occ_l1_kernel: the 1024-thread stride `for (k = threadIdx.x; k < cap; k += 1024)` (cap = 1, 1023, 1024, 1025, 4096), `if (i >= 0)`
    on the unused slots, `counts[0] > 1 ? counts[0] : 1` (kept = 0 with counts = (0, 0): no division by zero, loss exactly 0).
    occ_l1_bwd_kernel: `if (k >= cap) return`, `if (i < 0) return`, sgn(0) = 0 on the tie; nero_occ_l1_backward's memset of exactly n_in
    floats (n_in = 1, 4097, 70001) over a sentinel-filled d_occ."""
    L = _lib()
    q = G.l1_inputs(cap, kept, n_in)
    occ, cand, counts, gt = _cu(q['occ']), _cu(q['cand']), _cu(q['counts']), _cu(q['gt'])
    d_loss = _cu(torch.tensor([G.D_LOSS], dtype=F32))
    loss, d_occ = _f(1 + GUARD), _f(n_in + GUARD)
    L.check(L.lib.nero_occ_l1(_p(occ), _p(cand), _p(counts), _p(gt), cap, _p(loss), L.stream_ptr()))
    L.check(L.lib.nero_occ_l1_backward(_p(d_loss), _p(occ), _p(cand), _p(counts), _p(gt), cap, n_in, _p(d_occ), L.stream_ptr()))
    gl, gd = _take(loss, 1), _take(d_occ, n_in)
    (l64, d64), (l32, d32) = G.occ_l1_fwd_bwd(q), G.occ_l1_fwd_bwd(q, F32)
    report, fails = {}, []
    if kept == 0:
        assert float(gl) == 0.0 and bool((gd == 0).all())
    assert torch.equal(gd != 0, d64 != 0)                                  # zero outside the candidates and on the tie, nowhere else
    fails.append(_judge_loss(report, 'loss', gl[0], l64, l32, G.loss_bound(kept) if kept else 0.0, kept))
    fails.append(_judge(report, 'd_occ', gd, d64, d32, G.l1_floor()))
    _settle(f'step_glue_kernels::occ_l1[cap={cap},kept={kept},n_in={n_in}]', report, fails)


def test_occ_l1_refusals():
    """nero_occ_l1: `cap <= 0 || cap > PICK_MAX`; nero_occ_l1_backward: `cap <= 0 || n_in <= 0`, in front of its memset; NULL pointers"""
    L = _lib()
    lib = L.lib
    q = G.l1_inputs(4096, 4096, 4097)
    occ, cand, counts, gt = _cu(q['occ']), _cu(torch.cat([q['cand'], q['cand'][:1]])), _cu(q['counts']), _cu(torch.cat([q['gt'], q['gt'][:1]]))
    d_loss, loss, d_occ = _cu(torch.tensor([G.D_LOSS], dtype=F32)), _f(1 + GUARD), _f(4097 + GUARD)
    st = L.stream_ptr()
    b = [_p(occ), _p(cand), _p(counts), _p(gt), _p(loss)]
    assert lib.nero_occ_l1(b[0], b[1], b[2], b[3], 4097, b[4], st) == ERR_ARG
    assert lib.nero_occ_l1(b[0], b[1], b[2], b[3], 0, b[4], st) == ERR_ARG
    for k in range(5):
        a = list(b)
        a[k] = _p(None)
        assert lib.nero_occ_l1(a[0], a[1], a[2], a[3], 4096, a[4], st) == ERR_ARG, k
    b = [_p(d_loss), _p(occ), _p(cand), _p(counts), _p(gt), _p(d_occ)]
    assert lib.nero_occ_l1_backward(b[0], b[1], b[2], b[3], b[4], 0, 4097, b[5], st) == ERR_ARG
    assert lib.nero_occ_l1_backward(b[0], b[1], b[2], b[3], b[4], 4096, 0, b[5], st) == ERR_ARG
    for k in range(6):
        a = list(b)
        a[k] = _p(None)
        assert lib.nero_occ_l1_backward(a[0], a[1], a[2], a[3], a[4], 4096, 4097, a[5], st) == ERR_ARG, k
    torch.cuda.synchronize()
    assert _untouched(loss) and _untouched(d_occ)
    parity_report('step_glue_kernels::occ_l1_refusals', refused_calls=15)


# ---- 5. nero_shape_loss ---------------------------------------------------------------------------------------------------------------
def _shape_loss(L, dev, R, n_in, kind, w, with_occ):
    """one call on the current stream -> (losses [4], d_rgb [R,3], d_gerr [n_in], d_occ [n_in] | None) on the CPU; partials is exactly
    nero_shape_loss_partials(R, n_in) floats with a guard behind, and comes back fully written"""
    n_part = L.lib.nero_shape_loss_partials(R, n_in)
    assert n_part == 2 * (-(-max(R, n_in) // G.LB))
    losses, d_rgb, d_gerr, part = _f(4 + GUARD), _f(R + GUARD, 3), _f(n_in + GUARD), _f(n_part + GUARD)
    d_occ = _f(n_in + GUARD) if with_occ else None
    occ_args = [_p(dev[k] if with_occ else None) for k in ('occ', 'cand', 'counts', 'gt_occ')]
    L.check(L.lib.nero_shape_loss(R, kind, _p(dev['rgb']), _p(dev['gt']), n_in, _p(dev['gerr'] if n_in else None), C.c_float(G.EIK_W), *occ_args,
                                  _p(w), _p(losses), _p(d_rgb), _p(d_gerr), _p(d_occ), _p(part), L.stream_ptr()))
    torch.cuda.current_stream().synchronize()
    assert not bool((_take(part, n_part) == SENT).any()), 'a block partial was not written'
    return _take(losses, 4), _take(d_rgb, R), _take(d_gerr, n_in), (_take(d_occ, n_in) if with_occ else None)


@pytest.mark.parametrize('kind', range(4), ids=G.KINDS)
@pytest.mark.parametrize('R,n_in', G.LOSS_SHAPES)
def test_shape_loss(R, n_in, kind):
    """loss_rows_kernel: `if (i < R)` / `if (i < n_in)` with either side the longer one (255 / 257, 257 / 255, 256 / 256, one row, no inner
    sample), the four `kind` branches with a row rgb == gt (sgn(0) = 0, charbonier's 0 / sqrt(1e-3)) and rows at |df| == 0.25 in both signs
    (`if (a < beta)`: the joint takes the linear side), `w ? w[0] : 1.f`, `if (d_occ) d_occ[i] = 0.f` over a sentinel-filled d_occ.
    loss_final_kernel: `for (b = threadIdx.x; b < nb; b += LB)` with nb = 257 and 258 on the sample side and 258 on the ray side (a second
    strided round), `if (cand)`, `kept = counts[0]` = 0, 1 and 300, the tie occ == gt_occ, `n_in > 0 ? ... : 0.f`, `kept > 0 ? ... : 0.f`.
    Two runs and a run on a second stream give the same bits for losses, d_rgb, d_gerr and d_occ."""
    L = _lib()
    floors = G.loss_floors(kind)
    report, fails = {}, []
    for mode in G.occ_modes(n_in):
        q = G.loss_inputs(R, n_in, mode)
        dev = {k: _cu(v) for k, v in q.items()}
        bounds = G.loss_bounds(R, n_in, mode)
        kept = 0 if q['cand'] is None else int(q['counts'][0])
        for wi, w in enumerate(G.WEIGHTS):
            wd = None if w is None else _cu(torch.tensor(w, dtype=F32))
            run = lambda: _shape_loss(L, dev, R, n_in, kind, wd, mode != 'none')
            got, again, other = run(), run(), _second_stream(run)
            for a, b_, c in zip(got, again, other):
                assert (a is None and b_ is None and c is None) or (torch.equal(a, b_) and torch.equal(a, c)), 'runs differ'
            r64, r32 = G.loss_refs(R, n_in, mode, kind, wi), G.loss_refs(R, n_in, mode, kind, wi, F32)
            tag = f'[{mode},w={wi}]'
            for i, (nm, N) in enumerate((('total', max(R, n_in, kept)), ('loss_rgb', R), ('loss_eikonal', n_in), ('loss_occ', kept))):
                fails.append(_judge_loss(report, nm + tag, got[0][i], r64[0][i], r32[0][i], bounds[i], N))
            for i, nm in enumerate(('d_rgb', 'd_gerr', 'd_occ'), 1):
                if got[i] is None:
                    continue
                if got[i].numel():
                    fails.append(_judge(report, nm + tag, got[i], r64[i], r32[i], floors[nm]))
                assert torch.equal(got[i] != 0, r64[i] != 0), (nm, tag)      # exact zeros where the reference has them, nowhere else
            if mode != 'none':
                assert int((got[3] != 0).sum()) == max(kept - (kept >= 2), 0)   # d_occ fully overwritten: zero except at the candidates
    _settle(f'step_glue_kernels::shape_loss[R={R},n_in={n_in},{G.KINDS[kind]}]', report, fails)


def test_shape_loss_refusals():
    """nero_shape_loss: `R <= 0`, the range of rgb_kind, `n_in > 0 && (!gerr || !d_gerr)`, `cand && (... || !counts || ...)` and the NULL
    checks, all in front of the first launch: nothing is written"""
    L = _lib()
    lib = L.lib
    R, n_in = 257, 300
    q = G.loss_inputs(66000, 300, 'full')
    dev = {k: _cu(v) for k, v in q.items()}
    losses, d_rgb, d_gerr, d_occ, part = _f(4 + GUARD), _f(R + GUARD, 3), _f(n_in + GUARD), _f(n_in + GUARD), _f(lib.nero_shape_loss_partials(R, n_in) + GUARD)
    st = L.stream_ptr()
    names = ('rgb', 'gt', 'gerr', 'occ', 'cand', 'counts', 'gt_occ', 'losses', 'd_rgb', 'd_gerr', 'd_occ', 'part')
    base = dict(rgb=dev['rgb'], gt=dev['gt'], gerr=dev['gerr'], occ=dev['occ'], cand=dev['cand'], counts=dev['counts'], gt_occ=dev['gt_occ'],
                losses=losses, d_rgb=d_rgb, d_gerr=d_gerr, d_occ=d_occ, part=part)

    def call(R_=R, kind=0, n_in_=n_in, **null):
        a = {k: _p(None if k in null else base[k]) for k in names}
        return lib.nero_shape_loss(R_, kind, a['rgb'], a['gt'], n_in_, a['gerr'], C.c_float(G.EIK_W), a['occ'], a['cand'], a['counts'], a['gt_occ'],
                                   _p(None), a['losses'], a['d_rgb'], a['d_gerr'], a['d_occ'], a['part'], st)
    refused = 0
    for rc in (call(R_=0), call(R_=-1), call(kind=-1), call(kind=4), call(gerr=1), call(d_gerr=1), call(counts=1), call(gt_occ=1), call(occ=1),
               call(d_occ=1), call(n_in_=0), call(rgb=1), call(gt=1), call(losses=1), call(d_rgb=1), call(part=1)):
        assert rc == ERR_ARG, refused
        refused += 1
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in (losses, d_rgb, d_gerr, d_occ, part)), 'a refused call wrote to a buffer'
    assert lib.nero_shape_loss_partials(1, 0) == 2 and lib.nero_shape_loss_partials(256, 257) == 4 and lib.nero_shape_loss_partials(66000, 300) == 516
    parity_report('step_glue_kernels::shape_loss_refusals', refused_calls=refused)


# ---- 6. nero_var_grad -------------------------------------------------------------------------------------------------------------------
def test_var_grad():
    """var_grad_kernel: `expf(variance[0] * 10.0f)` over 64 variances in [-1.3, 1.3] (0.3 among them) with a dsum of either sign, and the
    gate `inv_s >= 1e-6f && inv_s <= 1e6f`: variance = 1.39 and -1.39 give exactly 0.0, 1.38 and -1.38 do not (no case within 1e-3 of
    ln(1e6) / 10, where a device expf one ulp off the host's would flip the step)"""
    L = _lib()
    v, s = G.var_grad_inputs()
    n = v.numel()
    vd, sd, grad = _cu(v), _cu(s), _f(n + GUARD)
    st = L.stream_ptr()
    for i in range(n):
        L.check(L.lib.nero_var_grad(_p(sd, 4 * i), _p(vd, 4 * i), _p(grad, 4 * i), st))
    got = _take(grad, n)
    g64, g32 = G.var_grad(s, v), G.var_grad(s, v, F32)
    for x, live in G.GATE_VARIANCES:
        rows = v == float(x)
        assert int(rows.sum()) == len(G.DSUMS) and bool(((got[rows] != 0) == live).all()), (float(x), got[rows].tolist())
    assert torch.equal(got != 0, g64 != 0)
    report = {}
    fails = [_judge(report, 'grad', got, g64, g32, G.var_grad_floor())]
    for k in range(3):
        a = [_p(sd), _p(vd), _p(grad, 4 * n)]
        a[k] = _p(None)
        assert L.lib.nero_var_grad(a[0], a[1], a[2], st) == ERR_ARG, k
    torch.cuda.synchronize()
    assert _untouched(grad[n:])
    _settle('step_glue_kernels::var_grad', report, fails)
