"""Plain-torch restatement of what nero_amd/chain.py::Chain computes, on the CPU and (by default) in float64: the reference of
tests/test_chain_kernels_gpu.py, pinned against torch autograd by tests/test_chain_ref_cpu.py.  It is driven by the same `entries` list
(Dense | None, Head | None) the product hands to Chain -- only the attributes are read (W, b, act, k_main, main_c0, k_aux, aux_c0, scale,
n_out; W, b, n_head, k) -- makes no GPU call and imports nothing from the kernels.

  forward     z_i = scale_i (W_i[:, main] x + W_i[:, aux] aux) + b_i,  a_i = act(z_i);  a head reads the INPUT tile of its entry
  reverse     delta_j = (sum over the entries fed by j of delta_i scale_i W_i[:, main] + dy_head W_head [+ dy]) act'(z_j) [+ inj_j]
              d_init = the same sum for the entries fed by `init`,  d_aux = sum_i delta_i scale_i W_i[:, aux]
  tangent     zdot_l = scale_l (W_l[:, main] adot_{l-1} + W_l[:, aux] auxdot),  adot_l = s_l zdot_l,  inj_l = gbar_l beta (1 - s_l) zdot_l
  weight_grads dW_i[:, part] = scale_i (delta_i^T in_part (+ D1^T B1_part)),  db_i = sum_r delta_i,  dWh = dy^T a_in (+ sum_r extra in row 0)

softplus is torch's softplus(beta=100, threshold=20): linear, with s = 1 exactly and no second derivative, where 100 z > 20.  s comes from
the pre-activation z of THIS forward, never from a saved output.

The second half of the file holds the cases both test files share: the shipped chain shapes at small row counts, their weights and inputs
from fixed seeds (`make_case`), and `reference_run`, which evaluates every tensor the GPU test compares -- in float64 as its reference, in
float32 as the arithmetic floor tests/test_chain_ref_cpu.py holds against the GPU test's bounds."""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
ACT_NONE, ACT_RELU, ACT_SOFTPLUS100 = 0, 1, 2                                # include/nero_hip.h NERO_ACT_*
BETA, THRESHOLD = 100.0, 20.0


def _t(x, dtype):
    return None if x is None else x.detach().to('cpu').to(dtype)


def _parts(d, dtype):
    """the two scaled column windows of a Dense: (W_main [n_out, k_main] or None, W_aux [n_out, k_aux] or None)"""
    W = _t(d.W, dtype)
    Wm = W[:, d.main_c0:d.main_c0 + d.k_main] * d.scale if d.k_main else None
    Wa = W[:, d.aux_c0:d.aux_c0 + d.k_aux] * d.scale if d.k_aux else None
    return Wm, Wa


def _prev_dense(entries):
    """per entry: the dense entry whose output is this entry's input tile (None: the init matrix)"""
    out, pd = [], None
    for i, (d, _) in enumerate(entries):
        out.append(pd)
        if d is not None:
            pd = i
    return out


def act_fn(act, z):
    if act == ACT_RELU:
        return F.relu(z)
    if act == ACT_SOFTPLUS100:
        return F.softplus(z, beta=BETA, threshold=THRESHOLD)
    assert act == ACT_NONE
    return z


def act_slope(act, z, gate=None):
    """act'(z); a ReLU layer takes `gate` (bool, the decisions of whoever ran the forward) when one is given"""
    if act == ACT_RELU:
        return (z > 0 if gate is None else gate).to(z.dtype)
    if act == ACT_SOFTPLUS100:
        return torch.where(BETA * z > THRESHOLD, torch.ones_like(z), torch.sigmoid(BETA * z))
    return torch.ones_like(z)


# ---- the four passes ----------------------------------------------------------------------------------------------------------------------
def forward(entries, init, aux=None, dtype=F64):
    """init [n, >= k of the first layer], aux [n, >= k_aux] -> dict(z=[per entry: pre-activation or None], a=[post-activation or None],
    heads={entry: [n, n_head]})"""
    x, A = _t(init, dtype), _t(aux, dtype)
    zs, acts, heads = [], [], {}
    for i, (d, h) in enumerate(entries):
        if h is not None:
            heads[i] = x[:, :h.k] @ _t(h.W, dtype).t() + (_t(h.b, dtype) if h.b is not None else 0)
        if d is None:
            zs.append(None)
            acts.append(None)
            continue
        Wm, Wa = _parts(d, dtype)
        z = torch.zeros(x.shape[0], d.n_out, dtype=dtype)
        if Wm is not None:
            z = z + x[:, :d.k_main] @ Wm.t()
        if Wa is not None:
            z = z + A[:, :d.k_aux] @ Wa.t()
        if d.b is not None:
            z = z + _t(d.b, dtype)
        x = act_fn(d.act, z)
        zs.append(z)
        acts.append(x)
    return {'z': zs, 'a': acts, 'heads': heads}


def reverse(entries, fwd, dy=None, head_dys=None, injs=None, gates=None, need_dinit=False, need_daux=False, accumulate_dinit=None,
            skip_last_dense=False, k_init=None, k_aux=None, dtype=F64):
    """dy: gradient w.r.t. the last dense entry's output (ACT_NONE) or, when the last entry is a head-only one, w.r.t. its input tile.
    head_dys {entry: [n, >= n_head]}, injs {dense entry: [n, >= n_out]} added to that entry's delta, gates {ReLU entry: bool [n, n_out]},
    accumulate_dinit: the matrix d_init is added onto.  -> dict(deltas={dense entry: [n, n_out]}, d_init [n, k_init], d_aux [n, k_aux])"""
    head_dys, injs, gates = head_dys or {}, injs or {}, gates or {}
    last, prev = len(entries) - 1, _prev_dense(entries)
    acc, deltas, d_aux = {}, {}, None                 # acc[j]: gradient w.r.t. the OUTPUT of dense entry j (None: w.r.t. init)

    def add(j, g):
        if j not in acc:
            acc[j] = torch.zeros(g.shape[0], k_init if j is None else entries[j][0].n_out, dtype=dtype)
        acc[j][:, :g.shape[1]] += g

    for i in range(last, -1, -1):
        d, h = entries[i]
        if d is not None and not (skip_last_dense and i == last):
            if i == last:
                assert d.act == ACT_NONE and dy is not None
                delta = _t(dy, dtype)[:, :d.n_out]
            else:
                delta = acc[i] * act_slope(d.act, fwd['z'][i], gates.get(i))
                if i in injs:
                    delta = delta + _t(injs[i], dtype)[:, :d.n_out]
            deltas[i] = delta
            Wm, Wa = _parts(d, dtype)
            if Wm is not None and (prev[i] is not None or need_dinit):
                add(prev[i], delta @ Wm)
            if Wa is not None and need_daux:
                d_aux = torch.zeros(delta.shape[0], k_aux, dtype=dtype) if d_aux is None else d_aux
                d_aux[:, :d.k_aux] += delta @ Wa
        elif d is None and i == last and dy is not None:
            add(prev[i], _t(dy, dtype)[:, :entries[prev[i]][0].n_out])
        if h is not None and i in head_dys and (prev[i] is not None or need_dinit):
            add(prev[i], _t(head_dys[i], dtype)[:, :h.n_head] @ _t(h.W, dtype))
    d_init = None
    if need_dinit:
        d_init = acc[None]
        if accumulate_dinit is not None:
            d_init = d_init + _t(accumulate_dinit, dtype)[:, :d_init.shape[1]]
    return {'deltas': deltas, 'd_init': d_init, 'd_aux': d_aux if need_daux else None}


def tangent(entries, fwd, init_dot, aux_dot=None, gbar=None, n_layers=None, dtype=F64, inj_beyond_threshold=False):
    """forward-mode pass of the first n_layers (softplus) entries: -> dict(zdot, adot, inj: lists; inj only with gbar {entry: [n, n_out]}).
    inj_beyond_threshold: a deliberately wrong variant (the linear region treated like the curved one) for the tests' mutation checks."""
    n_layers = len(entries) if n_layers is None else n_layers
    xd, Ad = _t(init_dot, dtype), _t(aux_dot, dtype)
    zdots, adots, injs = [], [], []
    for l in range(n_layers):
        d = entries[l][0]
        assert d is not None and d.act == ACT_SOFTPLUS100
        Wm, Wa = _parts(d, dtype)
        zdot = xd[:, :d.k_main] @ Wm.t()
        if Wa is not None:
            zdot = zdot + Ad[:, :d.k_aux] @ Wa.t()
        z = fwd['z'][l]
        s = act_slope(d.act, z)
        xd = s * zdot
        zdots.append(zdot)
        adots.append(xd)
        if gbar is not None:
            s2 = torch.sigmoid(BETA * z)
            inj = _t(gbar[l], dtype)[:, :d.n_out] * BETA * (1 - s2) * zdot
            if not inj_beyond_threshold:
                inj = torch.where(BETA * z > THRESHOLD, torch.zeros_like(inj), inj)
            injs.append(inj)
    return {'zdot': zdots, 'adot': adots, 'inj': injs}


def _rows_gemm(D, B, chunk=16):
    """D^T B summed over the rows in chunks of 16, the partial products then added up -- the order every row-sliced GEMM has.  float64 does not
    care; the float32 evaluation of tests/test_chain_ref_cpu.py does: one unblocked fp32 sum over 327 rows is at 0.2 - 0.46 of the 2e-6 bound"""
    return sum(D[r:r + chunk].t() @ B[r:r + chunk] for r in range(0, D.shape[0], chunk))


def weight_grads(entries, saves, deltas, init, aux=None, head_dys=None, second=None, head_extra=None, dtype=F64):
    """saves: per entry the layer's output (the GEMM's B operand of the next layer), deltas {dense entry: delta}, second {dense entry:
    (D1, B1_main, B1_aux)}, head_extra {entry: [n, >= k]} (include/nero_hip.h::nero_head_dw).  Every operand is used as given: all its rows.
    -> per entry dict(dW, db, dWh, dbh)"""
    head_dys, second, head_extra = head_dys or {}, second or {}, head_extra or {}
    prev, out = _prev_dense(entries), []
    for i, (d, h) in enumerate(entries):
        g = {}
        main_in = _t(init if prev[i] is None else saves[prev[i]], dtype)
        if h is not None and i in head_dys:
            dyh = _t(head_dys[i], dtype)[:, :h.n_head]
            g['dWh'] = _rows_gemm(dyh, main_in[:, :h.k])
            if i in head_extra:
                g['dWh'][0] += _t(head_extra[i], dtype)[:, :h.k].sum(0)
            g['dbh'] = dyh.sum(0)
        if d is not None:
            delta = _t(deltas[i], dtype)[:, :d.n_out]
            dW = torch.zeros(tuple(d.W.shape), dtype=dtype)
            sec = second.get(i)
            D1 = _t(sec[0], dtype)[:, :d.n_out] if sec is not None else None
            for which, (B, kc, c0) in enumerate(((main_in, d.k_main, d.main_c0), (_t(aux, dtype), d.k_aux, d.aux_c0))):
                if not kc:
                    continue
                part = _rows_gemm(delta, B[:, :kc])
                if sec is not None:
                    part = part + _rows_gemm(D1, _t(sec[1 + which], dtype)[:, :kc])
                dW[:, c0:c0 + kc] = d.scale * part
            g['dW'], g['db'] = dW, delta.sum(0)
        out.append(g)
    return out


# ---- norms and bounds of the comparison ----------------------------------------------------------------------------------------------------
def rel(a, b):
    """max|a - b| / max|b| in float64"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def rel_rows(a, b):
    """the largest per-ROW max|a - b| / max|b|: what a block scale taken per activation row keeps small and one taken per tile does not"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and a.dim() == 2
    return float(((a - b).abs().amax(1) / (b.abs().amax(1) + 1e-300)).max())


def bound(name):
    """the project's own figures: 2e-6 for a weight gradient from operands handed to the GEMM (tests/test_engines_extra.py on nero_dw_gemm),
    1e-4 for the second-order SDF weight gradients end to end and 2e-5 for every chain-pass output (tests/test_mlp_engine.py)"""
    if name.startswith('e2e.'):
        return 1e-4
    return 2e-6 if name.split('.')[-1].startswith(('dW', 'db')) else 2e-5


# ---- the shared cases ----------------------------------------------------------------------------------------------------------------------
ROWS = (1, 63, 64, 65, 129, 327)
SDF_SHAPES = {'sdf6': (6, 8), 'sdf4': (4, 6)}                                # name -> (sdf_freq, sdf_n_layers); sdf6 is every shipped YAML
LIGHTS = {'light24': (24, 3), 'light72': (72, 3), 'light90': (90, 3), 'light123': (123, 3), 'light144': (144, 3), 'light72_h1': (72, 1)}
CHAINS = tuple(SDF_SHAPES) + ('trunk', 'nerf_head', 'mat_h1', 'mat_h3') + tuple(LIGHTS) + ('feats',)
SCALED_ROWS = 129                                                            # the row-scaled forward case of every ReLU / identity chain


def row_pad(n):
    return (n + 63) // 64 * 64


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _lin(g, n_out, k, c, cb=0.1):
    return torch.randn(n_out, k, generator=g) * (c / math.sqrt(k)), torch.randn(n_out, generator=g) * cb


@functools.lru_cache(maxsize=None)
def weights(name):
    """the effective (W, b) list of chain `name`, float32 on the CPU, from a seed of its own: randn c / sqrt(k), small biases (c = 1.4 keeps a ReLU
    chain's activations level through the depth).  The softplus chains reach 100 z < -60 and 100 z > 20 through their BIASES, uniform over
    [-0.9, 0.5], on weights of c = 0.35: with the spread in the weights (c = 1.4, z ~ N(0, 0.3^2)) the float32 rounding of a 256-term
    pre-activation, times beta = 100, puts float32 torch itself at 0.55 - 0.6 of the 2e-5 bound on inj and on the deltas it enters"""
    g = torch.Generator().manual_seed(_seed('weights', name))
    if name in SDF_SHAPES:
        freq, n_layers = SDF_SHAPES[name]
        d_pe, skip = 3 + 6 * freq, n_layers // 2
        shapes = [(256 - d_pe if l == skip - 1 else (257 if l == n_layers else 256), d_pe if l == 0 else 256) for l in range(n_layers + 1)]
        eff = [_lin(g, o, k, 0.35, 0.05) for o, k in shapes]
        return [(W, torch.rand(b.shape[0], generator=g) * 1.4 - 0.9) for W, b in eff[:-1]] + eff[-1:]
    if name == 'trunk':                                                      # NeRF++: 8 x 256, [pe 84 | h 256] into layer 5, alpha head
        return [_lin(g, 256, 84 if i == 0 else (340 if i == 5 else 256), 1.4) for i in range(8)] + [_lin(g, 1, 256, 1.0)]
    if name == 'nerf_head':                                                  # feature, views, rgb
        return [_lin(g, 256, 256, 1.0), _lin(g, 128, 283, 1.4), _lin(g, 3, 128, 1.0)]
    if name in ('mat_h1', 'mat_h3'):
        return [_lin(g, 256, 259, 1.4), _lin(g, 256, 256, 1.4), _lin(g, 256, 256, 1.4), _lin(g, 1 if name == 'mat_h1' else 3, 256, 1.0)]
    if name in LIGHTS:
        k0, nh = LIGHTS[name]
        return [_lin(g, 256, k0, 1.4), _lin(g, 256, 256, 1.4), _lin(g, 256, 256, 1.4), _lin(g, nh, 256, 1.0)]
    assert name == 'feats'                                                   # MaterialFeatsNetwork: [h 256 | pe 51] into layer 4
    return [_lin(g, 256, 51 if i == 0 else (307 if i == 4 else 256), 1.4 if i < 7 else 1.0) for i in range(8)]


def build_entries(name, eff):
    """the entry list of chain `name` over the tensors of `eff` (on whatever device they are), by the product's builders where it has them,
    otherwise written as nero_amd/shape_step.py / material_step.py write them.  -> (entries, k_init, k_aux, aux_wide)"""
    from nero_amd.chain import Dense, Head
    from nero_amd.sdf import sdf_entries, sdf_shape
    from nero_amd.shape_step import predictor_entries
    if name in SDF_SHAPES:
        ld = sdf_shape(eff)[3]
        return sdf_entries(eff), ld, ld, False
    if name == 'trunk':
        ent = []
        for i, (W, b) in enumerate(eff[:8]):
            ent.append((Dense(W, b, ACT_RELU, 84) if i == 0 else Dense(W, b, ACT_RELU, 256, 84, 84, 0) if i == 5 else Dense(W, b, ACT_RELU, 256), None))
        return ent + [(None, Head(*eff[8]))], 88, 88, True
    if name == 'nerf_head':
        return [(Dense(*eff[0], ACT_NONE, 256), None), (Dense(*eff[1], ACT_RELU, 256, 0, 27, 256), None), (None, Head(*eff[2]))], 256, 32, False
    if name in ('mat_h1', 'mat_h3'):
        return predictor_entries(eff, 256, 3), 256, 8, False
    if name in LIGHTS:
        k0 = LIGHTS[name][0]
        return predictor_entries(eff, k0), (k0 + 7) // 8 * 8, 0, False
    ent = [(Dense(W, b, ACT_RELU, 51 if i == 0 else 256), None) for i, (W, b) in enumerate(eff[:4])]
    ent.append((Dense(*eff[4], ACT_RELU, 256, 0, 51, 256), None))
    ent += [(Dense(*eff[5], ACT_RELU, 256), None), (Dense(*eff[6], ACT_RELU, 256), None), (Dense(*eff[7], ACT_NONE, 256), None)]
    return ent, 56, 56, True


@functools.lru_cache(maxsize=None)
def make_case(name, n, scaled=False):
    """everything one GPU case is launched with, float32 on the CPU: the chain over weights(name) and, from a seed of (name, n), its inputs
    with all row_pad(n) rows finite and random -- the rows behind n belong to nobody and no output row < n may depend on them.  Columns
    between a matrix's logical and padded width are zero, as the product's encoders leave them.  scaled: the init rows times 2^k, k spread
    over [-20, 20] (forward only)."""
    g = torch.Generator().manual_seed(_seed('inputs', name, n, scaled))
    rp = row_pad(n)
    entries, k_init, k_aux, aux_wide = build_entries(name, weights(name))
    c = dict(name=name, n=n, rp=rp, entries=entries, k_init=k_init, k_aux=k_aux, aux_wide=aux_wide, scaled=scaled, sdf=name in SDF_SHAPES,
             aux=None, dy=None, head_dys={}, need_dinit=False, need_daux=False, onto=None)

    def rn(cols, used=None, amp=1.0):
        t = torch.zeros(rp, cols)
        t[:, :used or cols] = torch.randn(rp, used or cols, generator=g) * amp
        return t

    def grad_rows(cols, amp=1.0, mean=0.0):
        """an incoming gradient; a head's carries a mean, so that the single number a 1-row head's bias gradient is rests on no cancellation"""
        return (rn(cols) + mean) * amp
    last = len(entries) - 1
    if c['sdf']:
        d_pe = entries[0][0].k_main
        c['init'] = c['aux'] = rn(k_init, d_pe, 0.2)
        c['dy'], c['head_dys'] = grad_rows(256, 0.1), {last: grad_rows(4, mean=0.5)}
        c['ehat'] = rn(k_init, d_pe, 0.2)
        c['ones'] = torch.zeros(rp, 4)
        c['ones'][:, 0] = 1.0
    elif name == 'trunk':
        c['init'] = c['aux'] = rn(88, 84)
        c['dy'], c['head_dys'] = grad_rows(256, 0.1), {last: grad_rows(4, mean=0.5)}
    elif name == 'feats':
        c['init'] = c['aux'] = rn(56, 51)
        c['dy'] = grad_rows(256, 0.1)
    else:
        c['init'] = rn(k_init, entries[0][0].k_main)
        c['aux'] = rn(k_aux, entries[1][0].k_aux if name == 'nerf_head' else entries[0][0].k_aux) if k_aux else None
        c['head_dys'] = {last: grad_rows(4, mean=0.5)}
        c['need_dinit'], c['need_daux'], c['onto'] = True, bool(k_aux), rn(k_init)
    if scaled:
        assert not c['sdf']
        c['init'] = c['init'] * torch.exp2(torch.linspace(-20, 20, rp).round())[torch.randperm(rp, generator=g)][:, None]
        if c['aux'] is not None and name in ('trunk', 'feats'):
            c['aux'] = c['init']
    return c


def cases():
    """(name, n, scaled) of every GPU case"""
    return [(name, n, False) for name in CHAINS for n in ROWS] + [(name, SCALED_ROWS, True) for name in CHAINS if name not in SDF_SHAPES]


def softplus_regions(case):
    """(count of 100 z < -60, count of 100 z > 20) over the softplus layers' float64 pre-activations at the rows < n"""
    n = case['n']
    fw = forward(case['entries'], case['init'][:n], None if case['aux'] is None else case['aux'][:n])
    zs = [z for (d, _), z in zip(case['entries'], fw['z']) if d is not None and d.act == ACT_SOFTPLUS100]
    return sum(int((BETA * z < -60).sum()) for z in zs), sum(int((BETA * z > THRESHOLD).sum()) for z in zs)


def reference_run(case, dtype=F64, ops=None, mutate=''):
    """every tensor the GPU test compares for `case`, evaluated in `dtype` on the rows < n: {name: tensor}.

    ops: the operands a pass takes over from whoever ran the passes before it (the GPU test hands over the kernels' own), each optional --
      gates {ReLU entry: bool}            the forward's decisions, for the reverse passes
      gbar {entry: [n, 256]}              the normal pass's deltas, for the tangent pass's inj (SDF)
      dw = dict(saves, deltas, second, head_extra)   the weight-gradient GEMM's operands
    Missing ones are this evaluation's own.  The 'e2e.' gradients (SDF) always come from this evaluation's own passes, start to end.
    mutate: one deliberately wrong variant (tests/test_chain_ref_cpu.py::test_mutations_are_noticed)."""
    ops = ops or {}
    n, E, last = case['n'], case['entries'], len(case['entries']) - 1
    cut = lambda t: None if t is None else t[:n]
    init, aux, dy = cut(case['init']), cut(case['aux']), cut(case['dy'])
    hd = {i: cut(t) for i, t in case['head_dys'].items()}
    kw = dict(k_init=case['k_init'], k_aux=case['k_aux'], dtype=dtype)
    out = {}
    fw = forward(E, init, aux, dtype)
    for i, a in enumerate(fw['a']):
        if a is not None:
            out[f'save{i}'] = a
    for i, h in fw['heads'].items():
        out[f'head{i}'] = h
    if case['scaled']:
        return out
    gates = ops.get('gates') or {i: fw['z'][i] > 0 for i, (d, _) in enumerate(E) if d is not None and d.act == ACT_RELU}
    daux = case['need_daux'] and mutate != 'no_d_aux'

    def put(prefix, rv):
        for i, t in rv['deltas'].items():
            out[f'{prefix}delta{i}'] = t
        for k in ('d_init', 'd_aux'):
            if rv[k] is not None:
                out[prefix + k] = rv[k]
    if not case['sdf']:
        rv = reverse(E, fw, dy=dy, head_dys=hd, gates=gates, need_dinit=case['need_dinit'], need_daux=daux, **kw)
        if case['need_daux'] and not daux:
            rv['d_aux'] = torch.zeros(n, case['k_aux'], dtype=dtype)
        put('', rv)
        if case['onto'] is not None:
            onto = None if mutate == 'no_accumulate' else cut(case['onto'])
            out['acc.d_init'] = reverse(E, fw, dy=dy, head_dys=hd, gates=gates, need_dinit=True, accumulate_dinit=onto, **kw)['d_init']
        dw = ops.get('dw') or dict(saves=fw['a'], deltas=rv['deltas'])
        second = head_extra = None
    else:
        ehat, ones = cut(case['ehat']), cut(case['ones'])

        def sdf_passes(gbar_in=None):
            nrm = reverse(E, fw, head_dys={last: ones}, need_dinit=True, need_daux=True, skip_last_dense=True, **kw)
            gbar = gbar_in or nrm['deltas']
            tan = tangent(E, fw, ehat, ehat, gbar=gbar, n_layers=last, dtype=dtype, inj_beyond_threshold=mutate == 'inj_beyond_threshold')
            rv2 = reverse(E, fw, dy=dy, head_dys=hd, injs=dict(enumerate(tan['inj'])), **kw)
            return nrm, gbar, tan, rv2

        def sdf_second(gbar, adot):
            return ({l: (gbar[l], ehat if l == 0 else adot[l - 1], ehat) for l in range(last)}, {last: adot[last - 1]})
        put('rev1.', reverse(E, fw, dy=dy, head_dys=hd, **kw))
        nrm, gbar, tan, rv2 = sdf_passes(ops.get('gbar'))
        put('nrm.', nrm)
        for l in range(last):
            out[f'adot{l}'], out[f'inj{l}'] = tan['adot'][l], tan['inj'][l]
        put('rev2.', rv2)
        dw = ops.get('dw')
        if dw is None:
            second, head_extra = sdf_second(gbar, tan['adot'])
            dw = dict(saves=fw['a'], deltas=rv2['deltas'], second=second, head_extra=head_extra)
        if ops.get('gbar') is not None:
            nrm, gbar, tan, rv2 = sdf_passes()
        second, head_extra = sdf_second(gbar, tan['adot'])
        e2e = weight_grads(E, fw['a'], rv2['deltas'], init, aux, head_dys=hd, second=second, head_extra=head_extra, dtype=dtype)
        for i, g in enumerate(e2e):
            for k, t in g.items():
                out[f'e2e.{k}{i}'] = t
    gr = weight_grads(E, dw['saves'], dw['deltas'], init, aux, head_dys=hd, second=dw.get('second'), head_extra=dw.get('head_extra'), dtype=dtype)
    for i, g in enumerate(gr):
        for k, t in g.items():
            out[f'{k}{i}'] = t
    if mutate == 'pad_row_in_dw':                                            # row n, a pad row wherever n is no multiple of 64, joins the sums
        wide = reference_run(dict(case, n=n + 1), dtype)
        out.update({k: t for k, t in wide.items() if bound(k) == 2e-6})
    out['_ops'] = dict(gates=gates, gbar=gbar if case['sdf'] else None, dw=dw)
    return out


def compare(got, ref, scaled=False):
    """{name: (error, bound)} over every tensor of `ref`, in the norm the GPU test applies to it"""
    res = {}
    for k, b in ref.items():
        if k.startswith('_'):
            continue
        per_row = scaled and k.startswith('save')
        res[k] = ((rel_rows if per_row else rel)(got[k], b), bound(k))
    return res
