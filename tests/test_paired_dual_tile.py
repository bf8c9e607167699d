"""GPU tier: the dual-tile k-loop of the paired chain kernels (nero_amd/csrc/mlp_f16p.hip: a wave computes its two feature tiles w and
w + 4 in ONE walk over the k-steps, mlp_f16_util.h::gemm_f16x3_dual) against the 512-thread kernels (mlp_f16x3.hip), BIT FOR BIT, at
forced-paired size (NERO_F16_PAIRED bit 3).  The chains walk every branch of the loop selection:

  * 8 tiles per layer (256 wide): every wave on the dual loop;
  * 7 tiles (the SDF's 217-wide layer): wave 3 has no second tile and takes the single-tile loop, waves 0-2 the dual one;
  * 4 tiles (the 128-wide view layer): no wave has a second tile;
  * a narrow aux operand of 39 columns (the SDF skip layer), of 27 (the view layer) and of 3 (the material predictors): the aux k-steps
    convert the raw rows once for both tiles;
  * a first layer whose k_main is not a multiple of 32 (39 -> 48: an odd number of k-steps);
  * row counts that are not a multiple of 64, below and above the size at which two workgroups share every CU.

Forward: saves, ReLU sign words, head outputs.  The reverse and tangent passes of the same chains are compared the same way (deltas, input
gradients, the SDF normal and its second-order weight gradients): they share the operand images and the LDS planes with the forward pass."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1000, 100003]


@pytest.fixture
def paired():
    from nero_amd import chain as CH
    prev = CH.f16_paired()
    yield CH.f16_paired
    CH.f16_paired(prev)


def _rn(seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return lambda *s: torch.randn(*s, device='cuda', generator=g)


def _view_chain(n):
    """256 -> 256 (identity, 8 tiles) -> [256 | aux 27] -> 128 (ReLU, 4 tiles) -> head of 3"""
    from nero_amd import _lib as L
    from nero_amd.chain import Chain, Dense, Head, row_pad
    rn, rp = _rn(2), row_pad(n)
    ch = Chain([(Dense(rn(256, 256) / 16, rn(256) * 0.1, L.ACT_NONE, 256), None),
                (Dense(rn(128, 283) / 16, rn(128) * 0.1, L.ACT_RELU, 256, 0, 27, 256), None),
                (None, Head(rn(3, 128) / 8, rn(3) * 0.1))], k_init=256, k_aux=32).pack()
    return ch, rn(rp, 256), rn(rp, 32), 2, rn(rp, 4)


def _predictor_chain(n):
    """[256 | aux 3] -> 256 -> 256 -> 256 (ReLU, 8 tiles each) -> head of 1"""
    from nero_amd import _lib as L
    from nero_amd.chain import Chain, Dense, Head, row_pad
    rn, rp = _rn(3), row_pad(n)
    ch = Chain([(Dense(rn(256, 259) / 16, rn(256) * 0.1, L.ACT_RELU, 256, 0, 3, 256), None),
                (Dense(rn(256, 256) / 16, rn(256) * 0.1, L.ACT_RELU, 256), None),
                (Dense(rn(256, 256) / 16, rn(256) * 0.1, L.ACT_RELU, 256), None),
                (None, Head(rn(1, 256) / 8, rn(1) * 0.1))], k_init=256, k_aux=8).pack()
    return ch, rn(rp, 256), rn(rp, 8), 3, rn(rp, 4)


def _run_relu_chain(make, n):
    ch, init, aux, head, hdy = make(n)
    fwd = ch.forward(init, aux, n, save=True)
    out = {}
    for i, d in enumerate(ch.entries):
        if d[0] is not None:
            out[f'save{i}'] = fwd['saves'][i][:n, :d[0].n_out].clone()
            if fwd['masks'][i] is not None:
                out[f'mask{i}'] = fwd['masks'][i][:n, :(d[0].n_out + 31) // 32].clone()
    assert any(k.startswith('mask') for k in out)
    out['head'] = fwd['heads'][head][:n, :ch.entries[head][1].n_head].clone()
    bwd = ch.backward(fwd, n, dy=None, head_dys={head: hdy}, need_dinit=True, need_daux=True)
    for i, t in bwd['deltas'].items():
        out[f'delta{i}'] = t[:n, :ch.entries[i][0].n_out].clone()
    out['d_init'] = bwd['d_init'][:n].clone()
    out['d_aux'] = bwd['d_aux'][:n].clone()
    return out


def _same(cur, ref, what):
    assert cur.keys() == ref.keys()
    for k in ref:
        a, b = cur[k], ref[k]
        assert torch.equal(a, b), (what, k, int((a != b).sum()), float((a.float() - b.float()).abs().max()))


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('make', [_view_chain, _predictor_chain], ids=['view_128_aux27', 'predictor_256_aux3'])
def test_relu_chains_forward_and_reverse(paired, make, n):
    paired(0)
    ref = _run_relu_chain(make, n)
    assert all(bool(torch.isfinite(v.float()).all()) for v in ref.values())
    paired(8 | 7)
    for k in range(3):
        _same(_run_relu_chain(make, n), ref, k)


def _sdf_field():
    """the SDF network's shape: PE-6 input of 39 columns, 8 softplus layers of 256 with the 217-wide layer in front of the skip layer
    ([217 | aux 39] columns, scaled by 1 / sqrt 2), 257 outputs"""
    from nero_amd.sdf import SDFField
    rn = _rn(5)
    shapes = [(256, 39), (256, 256), (256, 256), (217, 256), (256, 256), (256, 256), (256, 256), (256, 256), (257, 256)]
    eff = [(rn(o, k) / math.sqrt(k), rn(o) * 0.05) for o, k in shapes]
    return SDFField(eff).pack()


def _run_sdf(field, n):
    from nero_amd.chain import row_pad
    rn, rp = _rn(7), row_pad(n)
    x = (rn(n, 3) * 0.5).contiguous()
    ctx = field.forward_normal(x, n)
    out = {'sdf': ctx['sdf4'][:n, 0].clone(), 'normal': ctx['normal'].clone()}
    for i, s in enumerate(ctx['fwd']['saves']):
        out[f'save{i}'] = s[:n, :field.full.entries[i][0].n_out].clone()
    for i, t in ctx['gbar'].items():
        if i < field.last:                             # (the normal pass skips the last dense layer: its delta buffer is never written)
            out[f'gbar{i}'] = t[:n, :field.full.entries[i][0].n_out].clone()
    d_sdf4 = torch.zeros(rp, 4, device='cuda')
    d_sdf4[:, 0] = rn(rp)
    grads = field.backward(ctx, d_sdf4, rn(rp, 256) * 0.1, (rn(n, 3) * 0.1).contiguous())
    for l, (dW, db) in enumerate(grads):
        out[f'dW{l}'], out[f'db{l}'] = dW.clone(), db.clone()
    return out


@pytest.mark.parametrize('n', ROWS)
def test_sdf_chain_forward_normal_tangent_and_reverse(paired, n):
    field = _sdf_field()
    paired(0)
    ref = _run_sdf(field, n)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    assert float(ref['normal'].abs().max()) > 0 and float(ref['dW3'].abs().max()) > 0
    paired(8 | 7)
    for k in range(3):
        _same(_run_sdf(field, n), ref, k)
