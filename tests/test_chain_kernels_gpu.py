"""GPU tier: every pass of the fused MLP-chain kernels (forward, reverse, tangent, weight-gradient GEMM) against the float64 reference
tests/chain_ref.py (pinned against autograd by tests/test_chain_ref_cpu.py), on every shipped chain shape -- the two SDF shapes, the NeRF++
trunk and head, the material predictors, the light predictors of every first-layer width, the material feature network -- at 1, 63, 64,
65, 129 and 327 rows, in all three arithmetics and, for f16x3, under the lock-step (nero_f16_paired(0)) and the paired (8 | 7) organisation.

A case runs the passes the product runs on that chain and compares EVERY output a later kernel reads: each layer's saved activation and
each head, each layer's delta, d_init and d_aux (also accumulated onto a random matrix), the SDF's normal pass (one-hot head seed,
skip_last_dense), the tangent's adot and inj per layer, the reverse pass with injections -- finished ones in f32 / bf16x6, formed by the
kernel from (gbar, adot) in f16x3 --, and dW / db / dWh / dbh of every entry, skip layers' two column parts, the SDF's second operand pair
and head_extra included.  The f16x3 sign words must decode to exactly `save > 0`.

Rows behind n hold finite random values in every input, and only rows < n are compared: no output row, and no weight gradient, may see them.
The reverse reference takes the KERNEL's ReLU decisions (a pre-activation within fp32 noise of 0 may land on either side), the tangent
reference the kernel's gbar, the weight-gradient reference the kernel's own saves and deltas as operands -- so a failure names the pass that
is wrong.  Bounds (chain_ref.bound): 2e-5 per tensor for every chain-pass output (per ROW for the saves of the case whose init rows are
scaled by 2^-20 .. 2^20: the fp16 planes are block-scaled per activation row), 2e-6 for a weight gradient from given operands, 1e-4 for the
SDF's second-order weight gradients end to end (then against the reference's own passes, start to end).  float32 torch sits within a third
of each on these very inputs (tests/test_chain_ref_cpu.py).  Every case appends its error per tensor to chain_fp64.json, beside the report of
tests/helpers.py::parity_report."""
import ctypes as C

import pytest
import torch

from tests import chain_ref as R
from tests.helpers import parity_report

pytestmark = pytest.mark.gpu


@pytest.fixture(params=['f32', 'bf16x6', 'f16x3'], autouse=True)
def gemm_mode(request):
    """every test runs on all dense-layer arithmetics (include/nero_hip.h NERO_GEMM_*): the exact fp32 MFMA, the 3-plane bf16 split and the
    2-plane block-scaled fp16 split, against the same float64 reference and the same bounds."""
    from nero_amd import chain
    old = dict(chain.GEMM_MODE)
    chain.set_gemm_mode(request.param)
    yield request.param
    chain.GEMM_MODE.update(old)


def gpu_chain(name):
    """the chain of `name` over chain_ref.weights(name) on the device, packed for the current arithmetic"""
    from nero_amd.chain import Chain
    eff = [(W.cuda(), b.cuda()) for W, b in R.weights(name)]
    entries, k_init, k_aux, aux_wide = R.build_entries(name, eff)
    return Chain(entries, k_init=k_init, k_aux=k_aux, aux_wide=aux_wide).pack()


def run_tangent(ch, fwd, ehat, n, n_layers, gbar):
    """the tangent chain as nero_amd.sdf.SDFField.backward describes it, in the current arithmetic.  gbar None: the injections are left to
    the reverse kernel (f16x3).  -> (adot per layer, inj per layer or None)"""
    from nero_amd import _lib as L
    from nero_amd.chain import GEMM_MODE, _r8, _r16, _tiles, row_pad
    mode = GEMM_MODE['tan']
    keys = {L.GEMM_F32: ('fm', 'fa'), L.GEMM_BF16X6: ('sfm', 'sfa'), L.GEMM_F16X3: ('hfm', 'hfa')}[mode]
    rk = _r8 if mode == L.GEMM_F32 else _r16
    rp = row_pad(n)
    tc = L.TanChain()
    tc.init, tc.ld_init, tc.k_init = ehat.data_ptr(), ehat.stride(0), ch.k_init
    tc.aux, tc.ld_aux, tc.k_aux = ehat.data_ptr(), ehat.stride(0), ch.k_aux
    tc.n_layers, tc.aux_wide, tc.gemm_mode = n_layers, 0, mode
    tc.macs_per_row = float(sum(ch.entries[l][0].n_out * (ch.entries[l][0].k_main + ch.entries[l][0].k_aux) for l in range(n_layers)))
    adot = torch.empty((n_layers, rp, L.HID), dtype=torch.float32, device='cuda')
    inj = torch.empty((n_layers, rp, L.HID), dtype=torch.float32, device='cuda') if gbar is not None else None
    for l in range(n_layers):
        d, p, tl = ch.entries[l][0], ch._packed[l], tc.layer[l]
        tl.w_main, tl.w_aux = L.ptr(p.get(keys[0])), L.ptr(p.get(keys[1]))
        tl.a_saved, tl.gbar = fwd['saves'][l].data_ptr(), (gbar[l].data_ptr() if gbar is not None else None)
        tl.adot, tl.inj = adot[l].data_ptr(), (inj[l].data_ptr() if gbar is not None else None)
        tl.k_main, tl.k_aux, tl.n_tiles = rk(d.k_main), (rk(d.k_aux) if d.k_aux else 0), _tiles(d.n_out)
    L.check(L.lib.nero_mlp_tangent(C.byref(tc), n, L.stream_ptr()))
    return adot, inj


def run_kernels(case, ch, mode):
    """-> (got {name: tensor, rows < n}, ops: what chain_ref.reference_run takes over from the kernels)"""
    from nero_amd import _lib as L
    from nero_amd.chain import decode_relu_masks
    n, E, last = case['n'], ch.entries, len(ch.entries) - 1
    init = case['init'].cuda()
    aux = init if case['aux'] is case['init'] else (None if case['aux'] is None else case['aux'].cuda())
    dy = None if case['dy'] is None else case['dy'].cuda()
    hd = {i: t.cuda() for i, t in case['head_dys'].items()}
    width = lambda i: E[i][0].n_out
    got = {}
    fwd = ch.forward(init, aux, n)
    for i, s in enumerate(fwd['saves']):
        if s is not None:
            got[f'save{i}'] = s[:n, :width(i)]
    for i, h in fwd['heads'].items():
        got[f'head{i}'] = h[:n, :E[i][1].n_head]
    relu = [i for i, (d, _) in enumerate(E) if d is not None and d.act == L.ACT_RELU]
    if mode == 'f16x3':                                  # the sign words and the save must tell the same story
        assert relu == [i for i, m in enumerate(fwd['masks']) if m is not None]
        for i in relu:
            dec = decode_relu_masks(fwd['masks'][i], n, width(i))
            assert torch.equal(dec, got[f'save{i}'] > 0), ('sign words', i, int((dec != (got[f'save{i}'] > 0)).sum()))
    if case['scaled']:
        return got, None
    ops = {'gates': {i: (got[f'save{i}'] > 0).cpu() for i in relu}}
    saves = [None if s is None else s[:n] for s in fwd['saves']]

    def put(prefix, bw, skip=()):
        for i, t in bw['deltas'].items():
            if i not in skip:
                got[f'{prefix}delta{i}'] = t[:n, :width(i)]
        for k in ('d_init', 'd_aux'):
            if bw[k] is not None:
                got[prefix + k] = bw[k][:n]
    if not case['sdf']:
        bwd = ch.backward(fwd, n, dy=dy, head_dys=hd, need_dinit=case['need_dinit'], need_daux=case['need_daux'])
        put('', bwd)
        if case['onto'] is not None:
            onto = case['onto'].cuda().clone()
            ch.backward(fwd, n, dy=dy, head_dys=hd, need_dinit=True, dinit_out=onto, accumulate_dinit=True)
            got['acc.d_init'] = onto[:n]
        gr = ch.weight_grads(fwd, bwd, n, init, aux, head_dys=hd)
        ops['dw'] = dict(saves=saves, deltas={i: t[:n] for i, t in bwd['deltas'].items()})
    else:
        ehat, ones = case['ehat'].cuda(), case['ones'].cuda()
        put('rev1.', ch.backward(fwd, n, dy=dy, head_dys=hd))
        nrm = ch.backward(fwd, n, dy=None, head_dys={last: ones}, need_dinit=True, need_daux=True, skip_last_dense=True)
        put('nrm.', nrm, skip=(last,))
        gbar = nrm['deltas']
        fused = mode == 'f16x3'                          # the reverse kernel forms the injections from (gbar, adot) itself
        adot, inj = run_tangent(ch, fwd, ehat, n, last, None if fused else gbar)
        for l in range(last):
            got[f'adot{l}'] = adot[l][:n, :width(l)]
            if not fused:
                got[f'inj{l}'] = inj[l][:n, :width(l)]
        rv2 = ch.backward(fwd, n, dy=dy, head_dys=hd, injs={l: (gbar[l], adot[l]) if fused else inj[l] for l in range(last)})
        put('rev2.', rv2)
        second = {l: (gbar[l], ehat if l == 0 else adot[l - 1], ehat) for l in range(last)}        # as SDFField.backward builds them
        head_extra = {last: adot[last - 1]}
        gr = ch.weight_grads(fwd, rv2, n, init, aux, head_dys=hd, second=second, head_extra=head_extra)
        ops['gbar'] = {l: gbar[l][:n] for l in range(last)}
        ops['dw'] = dict(saves=saves, deltas={i: t[:n] for i, t in rv2['deltas'].items()},
                         second={l: tuple(t[:n] for t in s) for l, s in second.items()}, head_extra={last: adot[last - 1][:n]})
    for i, g in enumerate(gr):
        for k, t in g.items():
            got[f'{k}{i}'] = t
            if case['sdf']:
                got[f'e2e.{k}{i}'] = t
    torch.cuda.synchronize()
    return got, ops


@pytest.mark.parametrize('name,n,scaled', R.cases(), ids=[f'{c}-{n}' + ('-rows_scaled' if s else '') for c, n, s in R.cases()])
def test_chain_passes_against_fp64(gemm_mode, name, n, scaled):
    from nero_amd import chain as CH
    case = R.make_case(name, n, scaled)
    if case['sdf']:
        lo, hi = R.softplus_regions(case)
        assert lo > 0 and hi > 0, ('both ends of the softplus must be populated', lo, hi)
    prev = CH.f16_paired()
    try:
        for org in ((0, 8 | 7) if gemm_mode == 'f16x3' else (None,)):
            if org is not None:
                CH.f16_paired(org)
            got, ops = run_kernels(case, gpu_chain(name), gemm_mode)
            ref = R.reference_run(case, R.F64, ops)
            fused = gemm_mode == 'f16x3'
            want = {k for k in ref if not k.startswith('_') and not (fused and k.startswith('inj'))}
            assert set(got) == want, sorted(set(got) ^ want)
            res = R.compare(got, {k: ref[k] for k in want}, scaled)
            parity_report(f'{name}-{n}' + ('-rows_scaled' if scaled else '') + f'[{gemm_mode}' + ('' if org is None else f',paired={org}') + ']',
                          file='chain_fp64.json', **{k: e for k, (e, b) in res.items()})
            bad = {k: (e, b) for k, (e, b) in res.items() if not e <= b}
            assert not bad, (name, n, gemm_mode, org, bad)
    finally:
        CH.f16_paired(prev)
