"""GPU tier: the kernels that turn gradients into the parameter update, called directly through the C ABI against tests/trainer_ref.py (pinned
by tests/test_trainer_ref_cpu.py): nero_wn_forward_batch, nero_wn_backward_batch and nero_wn_adam_batch (nero_amd/csrc/trainer.hip),
nero_head_dw / nero_head_dw_ld and the accumulate / scale / col0 branch of the weight-gradient reduction (nero_amd/csrc/mlp_engine.hip), at the
smallest shapes that cross each boundary: four rows per block and the 64-lane stride of the wave-per-row kernels, a full batch of 40 jobs with
unequal rows, the 96-job chunks of the plain Adam jobs and the grid-stride loop behind their 64-block cap, the 128-row slices, the 4- and
8-row unrolled strands and the four-group reduction of the head gradient.

Judged exactly as tests/test_shade_kernels_gpu.py judges Stage I (its helpers are imported): against the float64 reference evaluated on the
kernel's own float32 inputs, bound = max(3 x measured float32 floor, 8 float32 roundings), the floor being the float32 CPU evaluation of the
same reference over ALL cases of a family -- never the kernel.  A weight-norm matrix is judged per row, an Adam output and a head gradient
element by element; each against the larger of its own magnitude and the term size the reference states (tests/trainer_ref.py).  No element is
exempt and there is no outlier allowance.  Guards, inputs, skipped jobs, columns beyond k_cols, rows beyond n_head and everything a refused
call was handed are exact: all tensors of a call are carved from ONE sentinel-filled buffer whose every other float must come back bit for
bit.  Every measured figure goes to parity_report."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from tests import trainer_ref as T
from tests.helpers import parity_report
from tests.test_shade_kernels_gpu import (FLOOR_FACTOR, ROUNDINGS, SENT, _ALIVE, _judge, _lib, _release_inputs, _row_err, _settle)  # noqa: F401

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
GUARD = 8                                                                    # floats between two tensors of an arena (keeps 16-byte alignment)
ERR_ARG = -1
WN_OUT = ('w_eff', 'inv_norm', 'dv', 'dg')


# ---- the references and their float32 floors (CPU only: tests/test_trainer_ref_cpu.py runs the same judge on them) --------------------------
def wn_eval(w, dt, wrong=''):
    """the four weight-norm outputs of one input set in `dt`; the backward takes the float32 forward's inv_norm, as the kernel does"""
    v, g, dW = (w[k].to(dt) for k in ('v', 'g', 'dW'))
    w_eff, inv = T.wn_forward(v, g)
    inv_in = T.wn_forward(w['v'], w['g'])[1].to(dt)
    dv, dg, dvu, dgu = T.wn_backward(v, g, inv_in, dW, wrong)
    return dict(w_eff=w_eff, inv_norm=inv, dv=dv, dg=dg), dict(w_eff=0.0, inv_norm=0.0, dv=dvu, dg=dgu)


@functools.lru_cache(maxsize=None)
def wn_refs(rows, cols, seed=0):
    """-> name -> (float64 reference, float32 reference, unit)"""
    w = T.wn_inputs(rows, cols, seed)
    (r64, unit), (r32, _) = wn_eval(w, F64), wn_eval(w, F32)
    return {k: (r64[k], r32[k], unit[k]) for k in WN_OUT}


def wn_batch_keys():
    return [(r, c, 100 + i) for i, (r, c) in enumerate(T.WN_BATCH)]


@functools.lru_cache(maxsize=None)
def wn_floors():
    out = {}
    for key in [(r, c, 0) for r, c in T.WN_SHAPES] + wn_batch_keys():
        for name, (r64, r32, unit) in wn_refs(*key).items():
            out[name] = max(out.get(name, 0.0), _row_err(r32, r64, unit))
    return out


@functools.lru_cache(maxsize=None)
def adam_floors():
    """output -> the worst element of the float32 candidate over all cases and calls"""
    out = {}
    for ci in range(len(T.ADAM_CASES)):
        cand = T.adam_refs(ci)[1]
        for call in range(T.N_CALLS):
            for name in T.call_outputs(ci):
                r64, r32, unit = T.call_refs(ci, call, name)
                out[name] = max(out.get(name, 0.0), _row_err(T.flat(cand[call][name]), T.flat(r64), T.flat(unit)))
    return out


@functools.lru_cache(maxsize=None)
def head_floors():
    """(output, with extra) -> the worst element over all row counts of the full [4, 256] problem"""
    out = {}
    for rows, ex in itertools.product(T.HEAD_ROWS, (False, True)):
        r, uW, ub = T.head_refs(rows, ex)
        out['dWh', ex] = max(out.get(('dWh', ex), 0.0), _row_err(r[F32][0].reshape(-1), r[F64][0].reshape(-1), uW.reshape(-1)))
        out['dbh', ex] = max(out.get(('dbh', ex), 0.0), _row_err(r[F32][1], r[F64][1], ub))
    return out


def judge_elements(report, name, got, r64, r32, unit, floor):
    """_judge with every element its own row; of several judgements under one name the report keeps the worst"""
    u = T.flat(unit) if torch.is_tensor(unit) or isinstance(unit, (list, tuple)) else unit
    rep = {}
    fail = _judge(rep, name, T.flat(got), (T.flat(r64), T.flat(r32), u), floor)
    if name not in report or rep[name]['kernel'] >= report[name]['kernel']:
        report[name] = rep[name]
    return fail


# ---- one sentinel-filled buffer per call ---------------------------------------------------------------------------------------------------------
class Arena:
    """every tensor of a call carved from one float32 buffer filled with SENT, GUARD floats apart.  add() before build(); `image` is what the
    buffer must hold: everything a call may not write is compared with it bit for bit"""

    def __init__(self):
        self.parts, self.size, self.span = [], GUARD, {}

    def add(self, name, t):
        """t: a float32 cpu tensor, or the element count of an output (sentinel-filled) -> name"""
        n = t if isinstance(t, int) else t.numel()
        self.span[name] = (self.size, n)
        self.parts.append((self.size, None if isinstance(t, int) else t.reshape(-1).float()))
        self.size += (n + 3) // 4 * 4 + GUARD
        return name

    def build(self):
        self.image = torch.full((self.size,), SENT, dtype=F32)
        for off, t in self.parts:
            if t is not None:
                self.image[off:off + t.numel()] = t
        self.dev = self.image.cuda()
        _ALIVE.append(self.dev)
        return self

    def ptr(self, name, null=False):
        return C.c_void_p(None if null else self.addr(name))

    def addr(self, name):
        return self.dev.data_ptr() + 4 * self.span[name][0]

    def write(self, name, t):
        off, n = self.span[name]
        t = torch.full((n,), float(t)) if not torch.is_tensor(t) else t.reshape(-1).float()
        assert t.numel() == n
        self.image[off:off + n] = t
        self.dev[off:off + n] = t.cuda()

    def read(self, name):
        off, n = self.span[name]
        return self.dev[off:off + n].cpu()

    def settle(self, written=()):
        """after a call: everything outside the `written` tensors is bit for bit what it was; the written tensors become the new image.
        -> the snapshot (cpu)"""
        snap = self.dev.cpu()
        keep = torch.ones(self.size, dtype=torch.bool)
        for name in written:
            off, n = self.span[name]
            keep[off:off + n] = False
        same = snap.view(torch.int32) == self.image.view(torch.int32)
        bad = (keep & ~same).nonzero().reshape(-1)
        if bad.numel():
            owner = [k for k, (off, n) in self.span.items() if off <= int(bad[0]) < off + n]
            raise AssertionError(f'{bad.numel()} floats outside the outputs changed, the first at {int(bad[0])} ({owner or "a guard"})')
        self.image = snap.clone()
        return snap

    def take(self, snap, name, shape=None):
        off, n = self.span[name]
        return snap[off:off + n] if shape is None else snap[off:off + n].reshape(shape)


# ---- 1. weight-norm forward and backward: nero_wn_forward_batch / nero_wn_backward_batch ------------------------------------------------------
def _wn_arena(keys):
    """-> arena, the two job arrays (forward, backward) of the input sets `keys`"""
    L = _lib()
    A = Arena()
    for i, (rows, cols, seed) in enumerate(keys):
        w = T.wn_inputs(rows, cols, seed)
        for k in ('v', 'g', 'dW'):
            A.add(f'{k}{i}', w[k])
        A.add(f'inv_in{i}', wn_refs(rows, cols, seed)['inv_norm'][1])       # the float32 reference's own inv_norm: the backward's input
        for k, n in (('w_eff', rows * cols), ('inv_norm', rows), ('dv', rows * cols), ('dg', rows)):
            A.add(f'{k}{i}', n)
    A.build()
    fwd, bwd = (L.WnJob * len(keys))(), (L.WnGradJob * len(keys))()
    for i, (rows, cols, _) in enumerate(keys):
        f, b = fwd[i], bwd[i]
        f.v, f.g, f.w_eff, f.inv_norm, f.rows, f.cols = A.addr(f'v{i}'), A.addr(f'g{i}'), A.addr(f'w_eff{i}'), A.addr(f'inv_norm{i}'), rows, cols
        b.v, b.g, b.inv_norm, b.dW, b.dv, b.dg = (A.addr(f'{k}{i}') for k in ('v', 'g', 'inv_in', 'dW', 'dv', 'dg'))
        b.rows, b.cols = rows, cols
    return A, fwd, bwd


def _run_wn(test_id, keys):
    L = _lib()
    A, fwd, bwd = _wn_arena(keys)
    n = len(keys)
    L.check(L.lib.nero_wn_forward_batch(fwd, n, L.stream_ptr()))
    snap = A.settle([f'{k}{i}' for i in range(n) for k in ('w_eff', 'inv_norm')])
    L.check(L.lib.nero_wn_backward_batch(bwd, n, L.stream_ptr()))
    snap = A.settle([f'{k}{i}' for i in range(n) for k in ('dv', 'dg')])
    report, fails, floors = {}, [], wn_floors()
    for i, (rows, cols, seed) in enumerate(keys):
        refs = wn_refs(rows, cols, seed)
        for k in WN_OUT:
            got = A.take(snap, f'{k}{i}', refs[k][0].shape)
            rep = {}
            fails.append(_judge(rep, k, got, refs[k], floors[k]))
            if k not in report or rep[k]['kernel'] >= report[k]['kernel']:
                report[k] = dict(rep[k], worst_job=i)
    _settle(test_id, report, fails)


@pytest.mark.parametrize('rows,cols', T.WN_SHAPES)
def test_weight_norm_forward_backward_one_job(rows, cols):
    _run_wn(f'trainer_kernels::wn[rows={rows},cols={cols}]', [(rows, cols, 0)])


def test_weight_norm_forward_backward_full_batch():
    """NERO_MAX_WN_JOBS jobs with unequal rows in one call: the surplus blocks of the small jobs fall through"""
    keys = wn_batch_keys()
    assert len(keys) == T.MAX_WN_JOBS == _lib().MAX_WN_JOBS and len({r for r, _, _ in keys}) > 2
    _run_wn('trainer_kernels::wn[40 jobs]', keys)


# ---- 2. weight-norm backward fused with Adam, and plain Adam: nero_wn_adam_batch ------------------------------------------------------------------
def _adam_arena(inp, sizes):
    L = _lib()
    A = Arena()
    pl, off = inp['plain'], 0
    for j, n in enumerate(sizes):
        for k in 'pmv':
            A.add(f'{k}{j}', pl[k][off:off + n])
        A.add(f'grad{j}', n)
        off += n
    for i, w in enumerate(inp['wn']):
        for k in ('v', 'g', 'mv', 'vv', 'mg', 'vg'):
            A.add(f'wn.{k}{i}', w[k])
        for k, n in (('w_eff', w['rows'] * w['cols']), ('inv_norm', w['rows']), ('dW', w['rows'] * w['cols'])):
            A.add(f'wn.{k}{i}', n)
    A.build()
    plain = (L.AdamJob * max(len(sizes), 1))()
    for j, n in enumerate(sizes):
        plain[j].p, plain[j].grad, plain[j].m, plain[j].v, plain[j].n = A.addr(f'p{j}'), A.addr(f'grad{j}'), A.addr(f'm{j}'), A.addr(f'v{j}'), n
    wn = (L.WnJob * max(len(inp['wn']), 1))()
    for i, w in enumerate(inp['wn']):
        q = wn[i]
        q.v = q.v_rw = A.addr(f'wn.v{i}')
        q.g = q.g_rw = A.addr(f'wn.g{i}')
        q.w_eff, q.inv_norm, q.dW = A.addr(f'wn.w_eff{i}'), A.addr(f'wn.inv_norm{i}'), A.addr(f'wn.dW{i}')
        q.m_v, q.v_v, q.m_g, q.v_g = A.addr(f'wn.mv{i}'), A.addr(f'wn.vv{i}'), A.addr(f'wn.mg{i}'), A.addr(f'wn.vg{i}')
        q.rows, q.cols = w['rows'], w['cols']
    return A, plain, wn


@pytest.mark.parametrize('ci', range(len(T.ADAM_CASES)))
def test_adam_trajectory(ci):
    """eight consecutive calls with a fresh gradient each; p, m, v of every tensor judged after every call: a plain job against the float64
    trajectory from the same start, a weight-norm job against the float64 call on the state and inv_norm the kernels themselves left"""
    L = _lib()
    case, inp = T.ADAM_CASES[ci], T.adam_case_inputs(ci)
    sizes, n_wn, n_plain = case['plain'], len(case['wn']), len(case['plain'])
    A, plain, wn = _adam_arena(inp, sizes)
    floors, report, fails = adam_floors(), {}, []
    lr, b1, b2, eps = (C.c_float(x) for x in inp['hyper'])
    bounds = [0] + list(itertools.accumulate(sizes))
    skipped_calls = 0
    for call in range(T.N_CALLS):
        js = T.plain_job_steps(inp, call)[0].tolist()
        for j in range(n_plain):
            plain[j].step = js[j]
            A.write(f'grad{j}', inp['plain']['grads'][call][bounds[j]:bounds[j + 1]])
        for i, w in enumerate(inp['wn']):
            A.write(f'wn.dW{i}', w['dWs'][call])
        written = [f'{k}{j}' for j in range(n_plain) if js[j] >= 0 for k in 'pmv']      # a skipped job's p, m, v: bit for bit
        skipped_calls += sum(s < 0 for s in js)
        wn_refs_ = []
        if n_wn:
            L.check(L.lib.nero_wn_forward_batch(wn, n_wn, L.stream_ptr()))
            before = A.settle([f'wn.{k}{i}' for i in range(n_wn) for k in ('w_eff', 'inv_norm')])
            for i, w in enumerate(inp['wn']):
                shape = lambda k: (w['rows'], w['cols']) if k in ('v', 'mv', 'vv') else (w['rows'],)
                state = {k: A.take(before, f'wn.{k}{i}', shape(k)) for k in T.WN_KEYS}
                wn_refs_.append(T.wn_call_refs(state, A.take(before, f'wn.inv_norm{i}'), w['dWs'][call], inp['hyper'], inp['step0'] + call))
            written += [f'wn.{k}{i}' for i in range(n_wn) for k in T.WN_KEYS]
        L.check(L.lib.nero_wn_adam_batch(wn if n_wn else None, n_wn, plain if n_plain else None, n_plain, lr, b1, b2, eps, inp['step0'] + call,
                                         L.stream_ptr()))
        snap = A.settle(written)
        for name in T.call_outputs(ci):
            if name.startswith('plain.'):
                got = torch.cat([A.take(snap, f'{name[6:]}{j}') for j in range(n_plain)])
                ref = T.call_refs(ci, call, name)
            else:
                k = T.WN_KEYS[T.ADAM_OUT[3:].index(name)]
                got = torch.cat([A.take(snap, f'wn.{k}{i}') for i in range(n_wn)])
                ref = tuple([r[k][i] for r in wn_refs_] for i in range(3))
            fails.append(judge_elements(report, name, got, *ref, floors[name]))
    report['shape'] = dict(n_wn=n_wn, n_plain=n_plain, elements=int(sum(sizes)), skipped_job_calls=skipped_calls, first_step=inp['step0'])
    _settle(f'trainer_kernels::adam[case={ci}]', report, fails)


# ---- 3. head gradient: nero_head_dw / nero_head_dw_ld -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _workspace(n_rows):
    L = _lib()
    return torch.full((L.lib.nero_dw_workspace_floats(n_rows),), SENT, dtype=F32, device='cuda')


HEAD_CONFIGS = tuple(itertools.product(T.HEAD_N, (False, True), (True, False), T.HEAD_K, (0, 5)))   # n_head, extra, dbh, k_cols, ld - k_cols
HEAD_DST_ROWS = 4 + 3                                                       # the most head rows + guard rows of the same pitch


def one_rounding_of_sum(got, pre, res):
    """got == pre + res to one float32 rounding of that sum (a multiply by the scale contracted into the add rounds once, too)"""
    exact = pre.double() + res.double()
    return bool(((got.double() - exact).abs() <= T.EPS32 * exact.abs()).all())


@pytest.mark.parametrize('rows', T.HEAD_ROWS)
def test_head_gradient(rows):
    """every (n_head, extra, dbh, k_cols, pitch) at one row count.  dy columns at and beyond n_head and a / extra columns at and beyond k_cols
    hold finite foreign values; dWh has exactly n_head rows of k_cols columns, everything else of the destination stays as it was.  Then
    accumulate = 1 on a preloaded destination: preload + the accumulate = 0 result, to one rounding of the sum."""
    L = _lib()
    lib, st = L.lib, L.stream_ptr()
    h = T.head_inputs(rows)
    A = Arena()
    for k in ('dy', 'a', 'extra'):
        A.add(k, h[k])
    A.add('dWh', HEAD_DST_ROWS * 261)
    A.add('dbh', 8)
    A.build()
    g = T._gen(5)
    pre_W, pre_b = torch.randn(HEAD_DST_ROWS * 261, generator=g), torch.randn(8, generator=g)
    ws = _workspace(max(T.HEAD_ROWS))
    floors, report, fails = head_floors(), {}, []
    for n_head, ex, use_b, k, pad in HEAD_CONFIGS:
        ld = k + pad
        refs, uW, ub = T.head_refs(rows, ex)
        args = lambda acc: (A.ptr('dy'), A.ptr('a'), A.ptr('extra', null=not ex), n_head, rows, A.ptr('dWh'), ld, k, A.ptr('dbh', null=not use_b),
                            C.c_void_p(ws.data_ptr()), acc, st)
        A.write('dWh', SENT)
        A.write('dbh', SENT)
        L.check(lib.nero_head_dw_ld(*args(0)))
        W0, b0 = A.read('dWh'), A.read('dbh')
        live = torch.zeros(HEAD_DST_ROWS * 261, dtype=torch.bool)
        live[:HEAD_DST_ROWS * ld].reshape(HEAD_DST_ROWS, ld)[:n_head, :k] = True
        assert bool((W0[~live] == SENT).all()), ('dWh written outside its n_head x k_cols block', n_head, k, ld)
        assert bool((b0[n_head if use_b else 0:] == SENT).all()), ('dbh written beyond n_head, or though NULL', n_head, use_b)
        gW = W0[:HEAD_DST_ROWS * ld].reshape(HEAD_DST_ROWS, ld)[:n_head, :k]
        tag = '+extra' if ex else ''
        fails.append(judge_elements(report, 'dWh' + tag, gW, refs[F64][0][:n_head, :k], refs[F32][0][:n_head, :k], uW[:n_head, :k], floors['dWh', ex]))
        if use_b:
            fails.append(judge_elements(report, 'dbh' + tag, b0[:n_head], refs[F64][1][:n_head], refs[F32][1][:n_head], ub[:n_head], floors['dbh', ex]))
        if k == 256 and pad == 0:                                           # nero_head_dw IS the 256 / 256 form: bit for bit
            A.write('dWh', SENT)
            A.write('dbh', SENT)
            L.check(lib.nero_head_dw(*args(0)[:6], *args(0)[8:]))
            assert torch.equal(A.read('dWh'), W0) and torch.equal(A.read('dbh'), b0)
        A.write('dWh', pre_W)
        A.write('dbh', pre_b)
        L.check(lib.nero_head_dw_ld(*args(1)))
        W1, b1 = A.read('dWh'), A.read('dbh')
        assert torch.equal(W1[~live], pre_W[~live]) and torch.equal(b1[n_head if use_b else 0:], pre_b[n_head if use_b else 0:])
        assert one_rounding_of_sum(W1[live], pre_W[live], W0[live]), ('accumulate = 1: dWh', n_head, ex, k, ld)
        if use_b:
            assert one_rounding_of_sum(b1[:n_head], pre_b[:n_head], b0[:n_head]), ('accumulate = 1: dbh', n_head, ex)
        if rows == 0:
            assert torch.equal(W1, pre_W) and torch.equal(b1, pre_b), 'rows = 0 with accumulate = 1 changed the destination'
    A.write('dWh', SENT)
    A.write('dbh', SENT)
    A.settle()                                                               # dy, a, extra and every guard: untouched by all calls
    report['calls'] = dict(configs=len(HEAD_CONFIGS), rows=rows)
    _settle(f'trainer_kernels::head_dw[rows={rows}]', report, fails)


# ---- 4. weight gradient: accumulate, scale, col0 (the engines' own accuracy: tests/test_engines_extra.py) ---------------------------------------
@pytest.mark.parametrize('rows', [1, 17, 129])
@pytest.mark.parametrize('engine', ['F32', 'BF16X6', 'F16X3'])
def test_weight_gradient_accumulate_scale_col0(engine, rows):
    """a ragged 217 x 39 block written at col0 = 256 of a preloaded [256, 295] destination with scale = 0.5: accumulate = 1 gives preload + the
    accumulate = 0 result of the same job to one rounding of the sum; everything outside the block stays exact; db likewise, a NULL db untouched"""
    L = _lib()
    n_out, k, ldw, col0 = 217, 39, 295, 256
    g = T._gen(900 + rows)
    pad = (rows + 63) // 64 * 64
    D, B = torch.zeros(pad, 256), torch.zeros(pad, 256)
    D[:rows], B[:rows] = torch.randn(rows, 256, generator=g), torch.randn(rows, 256, generator=g)
    pre_W, pre_b = torch.randn(256, ldw, generator=g), torch.randn(256, generator=g)
    A = Arena()
    A.add('D', D), A.add('B', B), A.add('dW', pre_W), A.add('db', pre_b)
    A.build()
    ws = _workspace(max(T.HEAD_ROWS))
    job = L.DwJob()
    job.d0, job.ldd0, job.b0, job.ldb0 = A.addr('D'), 256, A.addr('B'), 256
    job.n_out, job.k_cols, job.dW, job.ldw, job.col0 = n_out, k, A.addr('dW'), ldw, col0
    job.scale, job.gemm_mode = 0.5, getattr(L, 'GEMM_' + engine)

    def run(accumulate, with_db):
        A.write('dW', pre_W)
        A.write('db', pre_b)
        job.accumulate, job.db = accumulate, A.addr('db') if with_db else None
        L.check(L.lib.nero_dw_gemm(C.byref(job), rows, C.c_void_p(ws.data_ptr()), L.stream_ptr()))
        snap = A.settle(['dW', 'db'])                                       # D, B and the guards: exact
        return A.take(snap, 'dW', (256, ldw)).clone(), A.take(snap, 'db').clone()
    live = torch.zeros(256, ldw, dtype=torch.bool)
    live[:n_out, col0:col0 + k] = True
    W0, b0 = run(0, True)
    assert torch.equal(W0[~live], pre_W[~live]) and torch.equal(b0[n_out:], pre_b[n_out:])
    assert bool((W0[live] != pre_W[live]).any()) and bool((b0[:n_out] != pre_b[:n_out]).all())
    W1, b1 = run(1, True)
    assert torch.equal(W1[~live], pre_W[~live]) and torch.equal(b1[n_out:], pre_b[n_out:])
    assert one_rounding_of_sum(W1[live], pre_W[live], W0[live]), 'accumulate = 1: dW is not preload + the accumulate = 0 result'
    assert one_rounding_of_sum(b1[:n_out], pre_b[:n_out], b0[:n_out]), 'accumulate = 1: db is not preload + the accumulate = 0 result'
    W2, b2 = run(1, False)
    assert torch.equal(W2, W1) and torch.equal(b2, pre_b), 'db == NULL: db written, or dW changed'
    parity_report(f'trainer_kernels::dw_accumulate[{engine},rows={rows}]', block=[n_out, k], col0=col0, ldw=ldw, scale=0.5,
                  accumulated_equal_bitwise=int((W1[live] == (pre_W[live] + W0[live])).sum()), elements=int(live.sum()))


# ---- 5. refusals before any launch: the argument error, and every buffer of the call bit for bit -------------------------------------------------
def test_refused_calls_change_nothing():
    L = _lib()
    lib, st = L.lib, L.stream_ptr()
    keys = [(5, 39, 0), (3, 65, 0)]
    A = Arena()
    for i, (rows, cols, seed) in enumerate(keys):
        w = T.wn_inputs(rows, cols, seed)
        for k in ('v', 'g', 'dW'):
            A.add(f'{k}{i}', w[k])
        A.add(f'inv{i}', wn_refs(rows, cols, seed)['inv_norm'][1])
        for k, n in (('w_eff', rows * cols), ('dv', rows * cols), ('dg', rows)):
            A.add(f'{k}{i}', n)
        for k, n in (('mv', rows * cols), ('vv', rows * cols), ('mg', rows), ('vg', rows)):
            A.add(f'{k}{i}', torch.zeros(n))
    for k in ('p', 'grad', 'm', 'v'):
        A.add(k, torch.full((300,), 0.25))
    A.build()

    def wn_jobs(n=2):
        jobs = (L.WnJob * n)()
        for q, i in zip(jobs, itertools.cycle(range(2))):
            q.v = q.v_rw = A.addr(f'v{i}')
            q.g = q.g_rw = A.addr(f'g{i}')
            q.w_eff, q.inv_norm, q.dW = A.addr(f'w_eff{i}'), A.addr(f'inv{i}'), A.addr(f'dW{i}')
            q.m_v, q.v_v, q.m_g, q.v_g = (A.addr(f'{k}{i}') for k in ('mv', 'vv', 'mg', 'vg'))
            q.rows, q.cols = keys[i][:2]
        return jobs

    def grad_jobs(n=2):
        jobs = (L.WnGradJob * n)()
        for q, i in zip(jobs, itertools.cycle(range(2))):
            q.v, q.g, q.inv_norm, q.dW, q.dv, q.dg = (A.addr(f'{k}{i}') for k in ('v', 'g', 'inv', 'dW', 'dv', 'dg'))
            q.rows, q.cols = keys[i][:2]
        return jobs

    def plain_jobs(n=1):
        jobs = (L.AdamJob * n)()
        for q in jobs:
            q.p, q.grad, q.m, q.v, q.n, q.step = A.addr('p'), A.addr('grad'), A.addr('m'), A.addr('v'), 300, 0
        return jobs

    def edit(jobs, i, **fields):
        for k, val in fields.items():
            setattr(jobs[i], k, val)
        return jobs
    hp = [C.c_float(x) for x in T.HYPERS[0]]
    adam = lambda wn, n_wn, pl, n_pl, step=3: lib.nero_wn_adam_batch(wn, n_wn, pl, n_pl, *hp, step, st)
    calls = {
        'forward: 41 jobs': lambda: lib.nero_wn_forward_batch(wn_jobs(41), 41, st),
        'backward: 41 jobs': lambda: lib.nero_wn_backward_batch(grad_jobs(41), 41, st),
        'adam: 41 weight-norm jobs': lambda: adam(wn_jobs(41), 41, plain_jobs(), 1),
        'adam: step 0': lambda: adam(wn_jobs(), 2, plain_jobs(), 1, step=0),
        'forward: NULL w_eff behind a valid job': lambda: lib.nero_wn_forward_batch(edit(wn_jobs(), 1, w_eff=None), 2, st),
        'forward: rows 0': lambda: lib.nero_wn_forward_batch(edit(wn_jobs(), 1, rows=0), 2, st),
        'forward: NULL array': lambda: lib.nero_wn_forward_batch(None, 2, st),
        'backward: NULL dg behind a valid job': lambda: lib.nero_wn_backward_batch(edit(grad_jobs(), 1, dg=None), 2, st),
        'backward: cols 0': lambda: lib.nero_wn_backward_batch(edit(grad_jobs(), 1, cols=0), 2, st),
        'backward: NULL array': lambda: lib.nero_wn_backward_batch(None, 2, st),
        'adam: NULL m_g behind a valid weight-norm job': lambda: adam(edit(wn_jobs(), 1, m_g=None), 2, plain_jobs(), 1),
        'adam: NULL dW': lambda: adam(edit(wn_jobs(), 0, dW=None), 2, None, 0),
        'adam: rows 0': lambda: adam(edit(wn_jobs(), 1, rows=0), 2, plain_jobs(), 1),
        'adam: cols 0': lambda: adam(edit(wn_jobs(), 0, cols=0), 2, None, 0),
        'adam: negative rows': lambda: adam(edit(wn_jobs(), 1, rows=-4), 2, None, 0),
        'adam: NULL weight-norm array': lambda: adam(None, 2, plain_jobs(), 1),
        'adam: NULL plain array': lambda: adam(wn_jobs(), 2, None, 1),
        'adam: NULL grad in a plain job behind valid weight-norm jobs': lambda: adam(wn_jobs(), 2, edit(plain_jobs(), 0, grad=None), 1),
        'adam: n 0 in the last of 98 plain jobs': lambda: adam(wn_jobs(), 2, edit(plain_jobs(98), 97, n=0), 98),
        'adam: negative plain count': lambda: adam(wn_jobs(), 2, plain_jobs(), -1),
    }
    for name, call in calls.items():
        assert call() == ERR_ARG, name
        assert lib.nero_last_error(), name
        A.settle()                                                           # nothing of the call's buffers changed: no launch was made
    parity_report('trainer_kernels::refusals', calls=len(calls))
