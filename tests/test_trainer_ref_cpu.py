"""CPU tier: pins tests/trainer_ref.py, the reference of tests/test_trainer_kernels_gpu.py, and proves on the CPU that the GPU tier's judge
would fail a subtly wrong kernel.
  (a) wn_forward / wn_backward in float64 against torch._weight_norm(v, g, 0) and its float64 autograd;
  (b) adam_step / wn_adam_step over N_CALLS = 8 steps against torch.optim.Adam on float64 CPU parameters: both hyper-parameter sets, first
      steps 1 and 25 000 (the bias corrections enter through the job's own step), a parameter whose .grad is None for the first three steps,
      one that never has a gradient;
  (c) head_dw against a float64 einsum;
  (d) the case tables cover what the issue names (n_plain 1 / 96 / 97 / 200 and 0, n_wn = 0, every plain size, skipped and own-step jobs on
      both sides of the 96-job chunk boundary, every gradient magnitude class);
  (e) each named wrong variant, evaluated in float32 and put through the GPU tier's own judge at the floors measured here, is rejected;
  (f) the float32 floors themselves, recorded with parity_report.
Bound of (a) - (c): agreement to float64 rounding.  Measured here, per element against the same units the GPU tier uses: 4e-16 (weight norm),
9e-16 (Adam against torch.optim.Adam, eight steps), 3e-16 (head gradient); asserted at 1e-13, a hundred float64 roundings and seven orders
below the float32 floors."""
import pytest
import torch

from tests import test_trainer_kernels_gpu as G
from tests import trainer_ref as T
from tests.helpers import parity_report
from tests.test_shade_kernels_gpu import FLOOR_FACTOR, ROUNDINGS, _judge, _row_err

F32, F64 = torch.float32, torch.float64
F64_BOUND = 1e-13


def _el(a, ref, unit=0.0):
    return _row_err(T.flat(a), T.flat(ref), T.flat(unit) if torch.is_tensor(unit) else unit)


# ---- (a) weight norm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols', [(1, 1), (3, 39), (5, 65), (217, 64), (257, 295)])
def test_weight_norm_reference_is_torch_weight_norm(rows, cols):
    w = {k: t.double() for k, t in T.wn_inputs(rows, cols).items()}
    v, g = w['v'].clone().requires_grad_(True), w['g'].reshape(rows, 1).clone().requires_grad_(True)
    W = torch._weight_norm(v, g, 0)
    W.backward(w['dW'])
    w_eff, inv = T.wn_forward(w['v'], w['g'])
    dv, dg, dvu, dgu = T.wn_backward(w['v'], w['g'], inv, w['dW'])
    assert _row_err(w_eff, W.detach()) <= F64_BOUND and _row_err(inv, 1.0 / w['v'].norm(dim=1)) <= F64_BOUND
    assert _el(dv, v.grad, dvu) <= F64_BOUND and _el(dg, g.grad.reshape(-1), dgu) <= F64_BOUND
    assert bool((dvu >= dv.abs() * (1 - 1e-12)).all()) and bool((dgu >= dg.abs() * (1 - 1e-12)).all())      # a unit bounds its output


# ---- (b) Adam ----------------------------------------------------------------------------------------------------------------------------------
def _torch_adam(params, hyper):
    lr, b1, b2, eps = hyper
    return torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, foreach=False)


@pytest.mark.parametrize('hi', range(len(T.HYPERS)))
def test_adam_reference_is_torch_adam(hi):
    """three tensors as one flat reference call: one on the call's step, one with no gradient for three steps that then counts its own, one
    that never has a gradient"""
    g = T._gen(11 + hi)
    n, hyper = 50, T.HYPERS[hi]
    p0 = torch.randn(3 * n, generator=g).double()
    grads = [T.draw_grad(3 * n, k, g).double() for k in range(T.N_CALLS)]
    ref = [p0[i * n:(i + 1) * n].clone().requires_grad_(True) for i in range(3)]
    opt = _torch_adam(ref, hyper)
    p, m, v, carry = p0.clone(), torch.zeros(3 * n, dtype=F64), torch.zeros(3 * n, dtype=F64), None
    worst = 0.0
    for call in range(T.N_CALLS):
        ref[0].grad = grads[call][:n].clone()
        ref[1].grad = None if call < 3 else grads[call][n:2 * n].clone()
        ref[2].grad = None
        opt.step()
        js = torch.tensor([0] * n + [T.job_step_of('late', call)] * n + [T.job_step_of('never', call)] * n)
        p, m, v, carry = T.adam_step(p, m, v, grads[call], *hyper, call + 1, js, carry=carry)
        want = torch.cat([t.detach() for t in ref])
        worst = max(worst, _el(p, want, carry['p']))
        st = opt.state[ref[0]]
        worst = max(worst, _el(m[:n], st['exp_avg'], carry['m'][:n]), _el(v[:n], st['exp_avg_sq'], carry['v'][:n]))
        if call >= 3:
            assert int(opt.state[ref[1]]['step']) == call - 2 == T.job_step_of('late', call)
    assert torch.equal(p[2 * n:], p0[2 * n:]) and not bool(m[2 * n:].any()) and not bool(v[2 * n:].any())
    assert worst <= F64_BOUND, worst
    print('adam_step against torch.optim.Adam, worst element:', worst)


def test_own_step_sets_the_bias_corrections():
    """job_step > 0 replaces the call's step: a late first step of 25 000 equals torch's 25 000th step on the same moments"""
    g = T._gen(3)
    hyper = T.HYPERS[0]
    p0, grad = torch.randn(40, generator=g).double(), T.draw_grad(40, 4, g).double()
    m0, v0 = 1e-3 * torch.randn(40, generator=g).double(), 1e-6 * torch.rand(40, generator=g).double()
    ref = p0.clone().requires_grad_(True)
    opt = _torch_adam([ref], hyper)
    opt.state[ref] = dict(step=torch.tensor(24999.0), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    ref.grad = grad.clone()
    opt.step()
    p, m, v, carry = T.adam_step(p0, m0, v0, grad, *hyper, 7, 25000)
    assert _el(p, ref.detach(), carry['p']) <= F64_BOUND
    same, _, _, _ = T.adam_step(p0, m0, v0, grad, *hyper, 25000, 0)
    assert torch.equal(same, p)
    wrong, _, _, _ = T.adam_step(p0, m0, v0, grad, *hyper, 7, 25000, wrong='call_step_for_own')
    assert _el(wrong, p, carry['p']) > 1e-3


@pytest.mark.parametrize('hi', range(len(T.HYPERS)))
def test_wn_adam_reference_is_torch_weight_norm_under_adam(hi):
    rows, cols, hyper = 5, 39, T.HYPERS[hi]
    w = {k: t.double() for k, t in T.wn_inputs(rows, cols, seed=3).items()}
    g = T._gen(21)
    dWs = [T.draw_grad(rows * cols, k, g).reshape(rows, cols).double() for k in range(T.N_CALLS)]
    rv, rg = w['v'].clone().requires_grad_(True), w['g'].reshape(rows, 1).clone().requires_grad_(True)
    opt = _torch_adam([rv, rg], hyper)
    z = lambda *s: torch.zeros(*s, dtype=F64)
    sv, sg, carry = (w['v'], z(rows, cols), z(rows, cols)), (w['g'], z(rows), z(rows)), None
    worst = 0.0
    for call in range(T.N_CALLS):
        opt.zero_grad()
        (torch._weight_norm(rv, rg, 0) * dWs[call]).sum().backward()
        opt.step()
        inv = T.wn_forward(sv[0], sg[0])[1]
        sv, sg, carry = T.wn_adam_step(sv[0], sg[0], inv, dWs[call], sv[1], sv[2], sg[1], sg[2], *hyper, call + 1, carry=carry)
        worst = max(worst, _el(sv[0], rv.detach(), carry['v']['p']), _el(sg[0], rg.detach().reshape(-1), carry['g']['p']),
                    _el(sv[1], opt.state[rv]['exp_avg'], carry['v']['m']), _el(sg[2], opt.state[rg]['exp_avg_sq'].reshape(-1), carry['g']['v']))
    assert worst <= F64_BOUND, worst
    print('wn_adam_step against torch, worst element:', worst)


# ---- (c) head gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [0, 1, 129, 2049])
def test_head_reference_is_einsum(rows):
    h = {k: t.double() for k, t in T.head_inputs(rows).items()}
    for n_head, k_cols, ex in ((1, 1, False), (3, 39, True), (4, 256, True), (2, 128, False)):
        dWh, dbh, uW, ub = T.head_dw(h['dy'], h['a'], h['extra'] if ex else None, n_head, k_cols)
        want = torch.einsum('rj,rk->jk', h['dy'][:, :n_head], h['a'][:, :k_cols])
        if ex:
            want[0] += h['extra'][:, :k_cols].sum(0)
        assert dWh.shape == (n_head, k_cols) and dbh.shape == (n_head,)
        assert _el(dWh, want, uW) <= F64_BOUND and _el(dbh, h['dy'][:, :n_head].sum(0), ub) <= F64_BOUND
        full, uF, _ = T.head_refs(rows, ex)                                  # every case is a slice of the full problem
        assert _el(full[F64][0][:n_head, :k_cols], want, uW) <= F64_BOUND and _el(uF[:n_head, :k_cols], uW) <= F64_BOUND


# ---- (d) the case tables -----------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_the_boundaries():
    assert set(T.WRONG) == set(T.ADAM_WRONG) | set(T.WN_WRONG) | {'extra_every_row'}          # each has a rejection test below
    assert len(T.WN_SHAPES) == 48 and len(T.WN_BATCH) == T.MAX_WN_JOBS
    assert {r for r, _ in T.WN_BATCH} == set(T.WN_ROWS) and {c for _, c in T.WN_BATCH} == set(T.WN_COLS)
    combos = {(c['hyper'], c['step0'], c['pscale']) for c in T.ADAM_CASES}
    assert len(combos) == 8 == len(T.ADAM_CASES)
    n_plain = {len(c['plain']) for c in T.ADAM_CASES}
    assert {0, 1, 96, 97, 200} <= n_plain and any(not c['wn'] and c['plain'] for c in T.ADAM_CASES)
    assert set(T.PLAIN_N) <= {n for c in T.ADAM_CASES for n in c['plain']}
    assert any(min(c['plain']) <= 3 and max(c['plain']) > 64 * 256 for c in T.ADAM_CASES if len(c['plain']) >= 96)
    for c in T.ADAM_CASES:
        kinds = T._plain_kinds(len(c['plain']))
        if len(c['plain']) > T.MAX_ADAM_JOBS:
            for side in (kinds[:96], kinds[96:]):                            # step < 0 and step > 0 on both sides of the chunk boundary
                steps = {T.job_step_of(k, call) for k in side for call in range(T.N_CALLS)}
                assert min(steps) < 0 < max(steps) and 0 in steps or len(side) == 1 and min(steps) < 0 < max(steps)
    assert any(cols < 64 for c in T.ADAM_CASES for _, cols in c['wn']) and any(cols > 64 for c in T.ADAM_CASES for _, cols in c['wn'])
    g = T.draw_grad(70, 0, T._gen(0))
    assert bool((g[7:14] == 0).all()) and bool((g[14:21].abs() == 1e-12).all()) and float(g[:7].abs().max()) <= 0.1354 < float(g[28:35].abs().max())
    assert T.draw_grad(1, 1, T._gen(0)).item() == 0 and abs(T.draw_grad(1, 2, T._gen(0)).item()) == T.c_float(1e-12)
    assert T.HYPERS[0][1:] == tuple(T.c_float(x) for x in (0.9, 0.999, 1e-8)) and all(a != b for a, b in zip(*T.HYPERS))
    for rows in T.HEAD_ROWS:                                                 # slices of the head kernel: 1 ... 5, 17 and a slice length off 128
        assert rows in (0, 1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 300, 512, 513, 2049, 33000)
    assert {(max(r, 1) + 127) // 128 for r in T.HEAD_ROWS if r <= 2049} >= {1, 2, 3, 4, 5, 17}


# ---- (e) the wrong variants are rejected by the GPU tier's judge at the measured floors -----------------------------------------------------------
def _rejected(name, got, ref, floor):
    """the GPU tier's verdict on `got`: a non-finite output is rejected by _judge's own assertion"""
    if not bool(torch.isfinite(T.flat(got)).all()):
        return True
    return G.judge_elements({}, name, got, *ref, floor) is not None


def _adam_verdicts(wrong):
    """-> the (case, call, output) triples on which the float32 evaluation of the wrong variant fails"""
    floors, hits = G.adam_floors(), []
    for ci in range(len(T.ADAM_CASES)):
        got = T.adam_trajectory(ci, F32, wrong)[0]
        for call in range(T.N_CALLS):
            for name in T.call_outputs(ci):
                if _rejected(name, got[call][name], T.call_refs(ci, call, name, got), floors[name]):
                    hits.append((ci, call, name))
    return hits


def test_the_correct_float32_reference_is_accepted():
    assert not _adam_verdicts('')
    floors = G.wn_floors()
    for rows, cols in T.WN_SHAPES:
        refs = G.wn_refs(rows, cols)
        assert all(_judge({}, k, refs[k][1], refs[k], floors[k]) is None for k in G.WN_OUT)


@pytest.mark.parametrize('wrong', T.ADAM_WRONG)
def test_wrong_adam_variants_are_rejected(wrong):
    hits = _adam_verdicts(wrong)
    assert hits, f'{wrong}: accepted on every case -- the bound is too loose or the inputs too tame'
    assert any(n.startswith('plain.') for _, _, n in hits)
    if wrong != 'call_step_for_own':                                         # (the weight-norm jobs have no step of their own)
        assert any(n.startswith('wn.') for _, _, n in hits)
    print(wrong, 'rejected on', len(hits), 'of the (case, call, output) triples, first', hits[0])


@pytest.mark.parametrize('wrong', T.WN_WRONG)
def test_wrong_weight_norm_variants_are_rejected(wrong):
    floors, hits = G.wn_floors(), []
    out = {'dv_no_projection': 'dv', 'dg_no_inv_norm': 'dg', 'c2_inv_first_power': 'dv'}[wrong]
    for rows, cols in T.WN_SHAPES:
        got = G.wn_eval(T.wn_inputs(rows, cols), F32, wrong)[0]
        refs = G.wn_refs(rows, cols)
        if _judge({}, out, got[out], refs[out], floors[out]) is not None:
            hits.append((rows, cols))
        assert all(torch.equal(got[k], refs[k][1]) for k in G.WN_OUT if k != out)
    # (with one column dv is zero in every variant but the one that drops the projection)
    assert len(hits) >= len([s for s in T.WN_SHAPES if s[1] > 1]), (wrong, hits)
    name = 'wn.g' if out == 'dg' else 'wn.v'                               # ... and through the fused Adam step
    assert any(n == name for _, _, n in _adam_verdicts(wrong)), wrong


def test_wrong_head_variant_is_rejected():
    floors = G.head_floors()
    for rows in (1, 129, 2049):
        h = T.head_inputs(rows)
        refs, uW, _ = T.head_refs(rows, True)
        for n_head in (2, 3, 4):
            got = T.head_dw(h['dy'], h['a'], h['extra'], n_head, 256, 'extra_every_row')[0]
            ref = (refs[F64][0][:n_head], refs[F32][0][:n_head], uW[:n_head])
            assert G.judge_elements({}, 'dWh', got, *ref, floors['dWh', True]) is not None, (rows, n_head)
            assert G.judge_elements({}, 'dWh', got[:1], *(t[:1] for t in ref), floors['dWh', True]) is None       # row 0 is right in both


def test_one_rounding_of_sum_is_one_rounding():
    g = T._gen(9)
    pre, res = torch.randn(4096, generator=g), torch.randn(4096, generator=g) * torch.exp(4 * torch.randn(4096, generator=g))
    assert G.one_rounding_of_sum(pre + res, pre, res)
    assert not G.one_rounding_of_sum(torch.nextafter(pre + res, torch.full((4096,), 1e30)), pre, res)
    assert not G.one_rounding_of_sum(pre + 2 * res, pre, res) and not G.one_rounding_of_sum(res, pre, res)


# ---- (f) the floors ---------------------------------------------------------------------------------------------------------------------------
def test_float32_floors_are_recorded():
    wn, adam, head = G.wn_floors(), G.adam_floors(), G.head_floors()
    bound = lambda f: max(FLOOR_FACTOR * f, ROUNDINGS * T.EPS32)
    parity_report('trainer_ref_cpu::float32_floors',
                  weight_norm={k: dict(fp32_floor=f, bound=bound(f)) for k, f in wn.items()},
                  adam={k: dict(fp32_floor=f, bound=bound(f)) for k, f in adam.items()},
                  head={f'{k}{"+extra" if ex else ""}': dict(fp32_floor=f, bound=bound(f)) for (k, ex), f in head.items()})
    # float32 grade: a floor of more than a few roundings per accumulated term would mean a unit that does not bound its output
    assert max(wn.values()) < 5e-7 and max(adam.values()) < 2e-6 and max(head.values()) < 2e-6, (wn, adam, head)
    assert set(adam) == set(T.ADAM_OUT)
