"""CPU tier: pins tests/chain_ref.py, the float64 reference of tests/test_chain_kernels_gpu.py, so that the GPU test does not compare two
things nobody checked.

  1. Against torch autograd in float64.  Every chain shape is written out once more as ordinary F.linear / relu / softplus code (`torch_net`,
     nothing shared with chain_ref), at 65 rows; first-order gradients by backward(), the SDF's normal pass and second-order weight gradients
     by autograd.grad(create_graph=True), the tangent by forward-mode AD.  chain_ref must agree to 1e-10 relative max-norm on EVERY tensor
     reference_run hands the GPU test (both sides are float64, only the summation order differs).
  2. The arithmetic floor of the GPU test's inputs: the same formulas in float32 torch, on the exact inputs of every GPU case (chain_ref.
     make_case), are within ONE THIRD of the bound the GPU test applies to each tensor, in the same norm.  That is what makes the GPU bounds
     firm; a tensor that misses it calls for other inputs (weight scale, seed), never for another bound.
  3. Each wrong variant the reference or the wiring could have is noticed by 1. or by the mask-word check."""
import copy
import math

import pytest
import torch
import torch.autograd.forward_ad as fwAD
import torch.nn.functional as F

from tests import chain_ref as R

F64 = torch.float64
PIN_ROWS, PIN_TOL = 65, 1e-10


def _build():
    import __graft_entry__ as ge
    ge.build()                                                               # the entry builders live in the package (host code only here)


# ---- the chains as ordinary torch code ------------------------------------------------------------------------------------------------------
def torch_net(name, P, x, aux):
    """P: list of (W, b).  -> (z per ENTRY of the product's chain, {entry: head output}, {entry: the head-only last entry's input})"""
    sp = lambda z: F.softplus(z, beta=100)
    if name in R.SDF_SHAPES:
        n_lin, d_pe = len(P), P[0][0].shape[1]
        skip, h, zs = (n_lin - 1) // 2, x[:, :d_pe], []
        for l, (W, b) in enumerate(P):
            if l == skip:
                h = torch.cat([h, aux[:, :d_pe]], -1) / math.sqrt(2)
            if l == n_lin - 1:
                return zs + [F.linear(h, W[1:], b[1:])], {l: F.linear(h, W[:1], b[:1])}, {}
            zs.append(F.linear(h, W, b))
            h = sp(zs[-1])
    if name == 'trunk':
        h, zs = x[:, :84], []
        for i, (W, b) in enumerate(P[:8]):
            if i == 5:
                h = torch.cat([aux[:, :84], h], -1)
            zs.append(F.linear(h, W, b))
            h = F.relu(zs[-1])
        return zs + [None], {8: F.linear(h, *P[8])}, {8: h}
    if name == 'nerf_head':
        z0 = F.linear(x, *P[0])
        z1 = F.linear(torch.cat([z0, aux[:, :27]], -1), *P[1])
        return [z0, z1, None], {2: F.linear(F.relu(z1), *P[2])}, {}
    if name == 'feats':
        h, zs = x[:, :51], []
        for i, (W, b) in enumerate(P):
            if i == 4:
                h = torch.cat([h, aux[:, :51]], -1)
            zs.append(F.linear(h, W, b))
            h = F.relu(zs[-1])
        return zs, {}, {}
    k0 = P[0][0].shape[1]                                                    # a predictor: layer 0 on [main | aux], then two layers and the head
    h = x[:, :k0] if aux is None else torch.cat([x, aux[:, :k0 - 256]], -1)
    zs = []
    for W, b in P[:3]:
        zs.append(F.linear(h, W, b))
        h = F.relu(zs[-1])
    return zs + [None], {3: F.linear(h, *P[3])}, {}


def autograd_run(name, case):
    """the tensors of chain_ref.reference_run(case), by autograd on torch_net"""
    n, E, last = case['n'], case['entries'], len(case['entries']) - 1
    leaf = lambda t: None if t is None else t[:n].double().clone().requires_grad_(True)
    cut = lambda t: None if t is None else t[:n].double()
    P = [(W.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)) for W, b in R.weights(name)]
    x, aux = leaf(case['init']), leaf(case['aux'])
    zs, heads, tile = torch_net(name, P, x, aux)
    for z in zs:
        if z is not None:
            z.retain_grad()
    out = {}
    for i, z in enumerate(zs):
        if z is not None:
            out[f'save{i}'] = R.act_fn(E[i][0].act, z).detach()
    for i, h in heads.items():
        out[f'head{i}'] = h.detach()
    dy, hd = cut(case['dy']), {i: cut(t) for i, t in case['head_dys'].items()}
    loss = sum((h * hd[i][:, :h.shape[1]]).sum() for i, h in heads.items())
    if dy is not None:
        target = zs[last] if zs[last] is not None else tile[last]
        loss = loss + (target * dy[:, :target.shape[1]]).sum()
    sdf = case['sdf']
    if sdf:
        dense = [z for z in zs if z is not None]
        for i, g in enumerate(torch.autograd.grad(loss, dense, retain_graph=True)):
            out[f'rev1.delta{i}'] = g
        g = torch.autograd.grad(heads[last][:, 0].sum(), [x, aux] + zs[:last], create_graph=True)
        out['nrm.d_init'], out['nrm.d_aux'] = g[0].detach(), g[1].detach()
        for l in range(last):
            out[f'nrm.delta{l}'] = g[2 + l].detach()
        ehat = cut(case['ehat'])
        loss = loss + ((g[0] + g[1]) * ehat).sum()
        for z in dense:
            z.grad = None                                                    # (autograd.grad fills the retained .grad too)
    loss.backward()
    pre = 'rev2.' if sdf else ''
    for i, z in enumerate(zs):
        if z is not None:
            out[f'{pre}delta{i}'] = z.grad
    if not sdf:
        if case['need_dinit']:
            out['d_init'] = x.grad
            out['acc.d_init'] = x.grad + cut(case['onto'])
        if case['need_daux']:
            out['d_aux'] = aux.grad
    for i, (d, h) in enumerate(E):                                           # the product's split of the effective weights into entries
        Wg, bg = P[i][0].grad, P[i][1].grad
        g = {}
        if sdf and i == last:
            g = {'dW': Wg[1:], 'db': bg[1:], 'dWh': Wg[:1], 'dbh': bg[:1]}
        elif d is not None:
            g = {'dW': Wg, 'db': bg}
        else:
            g = {'dWh': Wg, 'dbh': bg}
        for k, t in g.items():
            out[f'{k}{i}'] = t
            if sdf:
                out[f'e2e.{k}{i}'] = t
    if sdf:                                                                  # the tangent of every layer's output along ehat, forward mode
        with fwAD.dual_level():
            Pd = [(W.detach(), b.detach()) for W, b in P]
            e = fwAD.make_dual(x.detach(), ehat)
            zd, _, _ = torch_net(name, Pd, e, e)
            for l in range(last):
                out[f'adot{l}'] = fwAD.unpack_dual(F.softplus(zd[l], beta=100)).tangent
                # inj_l = u_l s'(z_l) zdot_l with u_l = gbar_l / s_l: s and s' are autograd's first and second derivative of torch's softplus
                z = zs[l].detach().requires_grad_(True)
                (s,) = torch.autograd.grad(F.softplus(z, beta=100).sum(), z, create_graph=True)
                (s1,) = torch.autograd.grad(s.sum(), z)
                out[f'inj{l}'] = out[f'nrm.delta{l}'] * (s1 / s.detach()) * fwAD.unpack_dual(zd[l]).tangent.detach()
    gates = {i: zs[i].detach() > 0 for i, (d, _) in enumerate(E) if d is not None and d.act == R.ACT_RELU}
    return out, gates


def pin_errors(name, case=None, mutate=''):
    """{tensor: relative max-norm error of chain_ref against autograd}; the reverse passes take AUTOGRAD's ReLU gates"""
    case = case or R.make_case(name, PIN_ROWS)
    want, gates = autograd_run(name, R.make_case(name, PIN_ROWS))
    got = R.reference_run(case, F64, ops={'gates': gates}, mutate=mutate)
    missing = [k for k in got if not k.startswith('_') and k not in want]
    assert not missing, missing
    return {k: R.rel(got[k], want[k]) for k in want}


@pytest.mark.parametrize('name', R.CHAINS)
def test_reference_agrees_with_autograd_in_fp64(name):
    _build()
    err = pin_errors(name)
    bad = {k: e for k, e in err.items() if not e <= PIN_TOL}
    assert not bad, bad
    kinds = {k.rstrip('0123456789') for k in err}
    assert {'save', 'dW', 'db'} <= kinds and (('rev2.delta' in kinds and 'adot' in kinds and 'inj' in kinds and 'nrm.d_aux' in kinds) if name in R.SDF_SHAPES else 'delta' in kinds)


@pytest.mark.parametrize('name', sorted(R.SDF_SHAPES))
def test_sdf_torch_net_is_the_oracles_network(name):
    """the hand-written SDF network above is oracle.nero_oracle.sdf_network, fed a real position encoding"""
    from oracle import nero_oracle as O
    eff = [(W.double(), b.double()) for W, b in R.weights(name)]
    P = {f'sdf_network.lin{l}.weight': W for l, (W, _) in enumerate(eff)}
    P.update({f'sdf_network.lin{l}.bias': b for l, (_, b) in enumerate(eff)})
    x = torch.rand(PIN_ROWS, 3, generator=torch.Generator().manual_seed(7), dtype=F64) * 1.6 - 0.8
    e = O.pos_enc(x, R.SDF_SHAPES[name][0])
    zs, heads, _ = torch_net(name, eff, e, e)
    y = O.sdf_network(P, x)
    assert R.rel(heads[len(eff) - 1], y[:, :1]) < 1e-12 and R.rel(zs[-1], y[:, 1:]) < 1e-12


# ---- the float32 floor of every GPU case ----------------------------------------------------------------------------------------------------
def _to32(x):
    if isinstance(x, torch.Tensor):
        return x if x.dtype == torch.bool else x.float()
    if isinstance(x, dict):
        return {k: _to32(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to32(v) for v in x)
    return x


@pytest.mark.parametrize('name', R.CHAINS)
def test_fp32_torch_is_within_a_third_of_every_gpu_bound(name):
    """for every GPU case of this chain (all row counts, the row-scaled one): the float32 evaluation, handed the same float32 operands the
    float64 one gets, misses no tensor by more than a third of its bound"""
    _build()
    worst, bad = {}, {}
    for nm, n, scaled in R.cases():
        if nm != name:
            continue
        case = R.make_case(nm, n, scaled)
        ops = _to32(R.reference_run(case, F64)['_ops']) if not scaled else None
        ref, flo = R.reference_run(case, F64, ops), R.reference_run(case, torch.float32, ops)
        for k, (e, b) in R.compare(flo, ref, scaled).items():
            worst[k.rstrip('0123456789')] = max(worst.get(k.rstrip('0123456789'), 0.0), e / b)
            if not e <= b / 3:
                bad[(n, scaled, k)] = (e, b)
        if case['sdf']:
            lo, hi = R.softplus_regions(case)
            assert lo > 0 and hi > 0, (nm, n, lo, hi)
    print(name, {k: round(v, 3) for k, v in sorted(worst.items())})
    assert not bad, bad


# ---- wrong variants are noticed ---------------------------------------------------------------------------------------------------------------
def _rewired(name, edit):
    case = dict(R.make_case(name, PIN_ROWS))
    case['entries'] = [(copy.copy(d), h) for d, h in case['entries']]
    edit(case['entries'])
    return case


def _no_skip_scale(entries):
    d = next(d for d, _ in entries if d is not None and d.scale != 1.0)
    d.scale = 1.0


def _swap_trunk_windows(entries):
    d = entries[5][0]
    d.main_c0, d.aux_c0 = d.aux_c0, d.main_c0


MUTATIONS = {'no_skip_scale': ('sdf6', _no_skip_scale, ''), 'swap_trunk_windows': ('trunk', _swap_trunk_windows, ''),
             'no_d_aux': ('mat_h3', None, 'no_d_aux'), 'no_accumulate': ('nerf_head', None, 'no_accumulate'),
             'inj_beyond_threshold': ('sdf4', None, 'inj_beyond_threshold'), 'pad_row_in_dw': ('light90', None, 'pad_row_in_dw')}


@pytest.mark.parametrize('which', sorted(MUTATIONS))
def test_mutations_are_noticed(which):
    """each wrong variant of the reference (or of the entry list it is driven by) breaks the autograd pin, by ten times its tolerance at the least"""
    _build()
    name, edit, mutate = MUTATIONS[which]
    err = pin_errors(name, _rewired(name, edit) if edit else None, mutate)
    assert max(err.values()) > 10 * PIN_TOL, (which, max(err.values()))


def _encode_relu_masks(gate):
    """bool [n, n_out] -> int32 [n, 8] sign words by the layout include/nero_hip.h documents for nero_fwd_layer.relu_mask: bit 16 h + v of
    word [row][tile] is output 32 tile + 4 h + (v & 3) + 8 (v >> 2)"""
    n, n_out = gate.shape
    full = torch.zeros(n, 256, dtype=torch.int64)
    full[:, :n_out] = gate.long()
    words = torch.zeros(n, 8, dtype=torch.int64)
    for h in range(2):
        for v in range(16):
            words |= full[:, torch.arange(8) * 32 + 4 * h + (v & 3) + 8 * (v >> 2)] << (16 * h + v)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


@pytest.mark.parametrize('n_out', [256, 217, 128])
def test_mask_decode_reads_the_documented_word_layout(n_out):
    """nero_amd.chain.decode_relu_masks, which the GPU test holds against `save > 0`, is the inverse of the header's layout -- and a decode
    that is one bit off is not"""
    _build()
    from nero_amd.chain import decode_relu_masks
    gate = torch.rand(65, n_out, generator=torch.Generator().manual_seed(n_out)) < 0.5
    words = _encode_relu_masks(gate)
    assert torch.equal(decode_relu_masks(words, 65, n_out), gate)
    assert not torch.equal(decode_relu_masks(words >> 1, 65, n_out), gate)
