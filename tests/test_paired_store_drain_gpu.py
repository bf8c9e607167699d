"""GPU tier: the paired chain kernels (nero_amd/csrc/mlp_f16p.hip) with their weight ring prefilled in front of the row stores and their
hand-counted vmcnt waits, against the lock-step kernels (mlp_f16x3.hip, untouched): every output a later kernel reads, BIT FOR BIT, at the
row counts where a reordered store or a wait that is one request short shows (1, 63, 64, 65, 129, 327: one lane, a tile minus one, a full
tile, a tile plus one, two tiles plus one, an odd count over several workgroups), on chains that walk every loop selection of the paired
kernels:
  * a predictor: 8-column aux on layer 0, three 256-wide ReLU layers (sign words), a 3-wide head -> the run of plain layers, the
    mask-only reverse, d_init / d_aux;
  * an SDF-shaped softplus chain (sdf_entries: the 217-wide layer -- wave 3 without a second tile --, the 39-column skip aux) -> forward,
    tangent, and the reverse with injections formed from (gbar, adot);
  * a NeRF-head chain 256 -> 256 -> 128 (+ 27-column aux) -> 3: n_tiles <= 4, single-tile loops.
Every launch runs twice (equal), and every workspace has 64 sentinel rows behind row_pad(n) that must stay untouched."""
import contextlib
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 129, 327]
SENT_F, SENT_I, GUARD = -12345.0, 0x5A5A5A5A, 64


@pytest.fixture
def paired():
    from nero_amd import chain as CH
    prev = CH.f16_paired()
    yield CH.f16_paired
    CH.f16_paired(prev)


class _GuardedTorch:
    """stands in for `torch` inside nero_amd.chain: every [.., rows, width] workspace Chain.forward / .backward allocates gets GUARD sentinel
    rows behind its rows (behind EVERY layer's rows of a stacked buffer); everything else is torch's"""

    def __init__(self):
        self.full = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device, zero):
        shape = tuple(shape)
        big = shape[:-2] + (shape[-2] + GUARD, shape[-1])
        t = torch.full(big, SENT_I if dtype == torch.int32 else SENT_F, dtype=dtype, device=device)
        view = t.narrow(-2, 0, shape[-2])
        if zero:
            view.zero_()
        self.full.append((t, shape[-2]))
        return view

    def empty(self, shape, dtype=torch.float32, device=None):
        if isinstance(shape, (tuple, list)) and len(shape) >= 2:
            return self._alloc(shape, dtype, device, False)
        return torch.empty(shape, dtype=dtype, device=device)

    def zeros(self, shape, dtype=torch.float32, device=None):
        if isinstance(shape, (tuple, list)) and len(shape) >= 2:
            return self._alloc(shape, dtype, device, True)
        return torch.zeros(shape, dtype=dtype, device=device)

    def check(self):
        for t, rows in self.full:
            tail = t.narrow(-2, rows, GUARD)
            want = SENT_I if t.dtype == torch.int32 else SENT_F
            assert bool((tail == want).all()), ('sentinel rows written', tuple(t.shape), rows)


@contextlib.contextmanager
def guarded():
    from nero_amd import chain as CH
    g = _GuardedTorch()
    CH.torch = g
    try:
        yield g
    finally:
        CH.torch = torch


def guarded_rows(rows, width, fill=None):
    """a caller-owned [rows + GUARD, width] workspace: (view of the rows, full tensor)"""
    t = torch.full((rows + GUARD, width), SENT_F, dtype=torch.float32, device='cuda')
    if fill is not None:
        t[:rows] = fill
    return t[:rows], t


def rn(g, *s):
    return torch.randn(*s, device='cuda', generator=g)


def same(a, b, what):
    assert torch.equal(a, b), (what, int((a != b).sum()), float((a.float() - b.float()).abs().max()))


# ---- the chains -------------------------------------------------------------------------------------------------------------------------
def predictor_chain(g):
    from nero_amd import _lib as L
    from nero_amd.chain import Chain, Dense, Head
    W0, b0 = rn(g, 256, 264) / 16, rn(g, 256) * 0.1
    W1, b1 = rn(g, 256, 256) / 16, rn(g, 256) * 0.1
    W2, b2 = rn(g, 256, 256) / 16, rn(g, 256) * 0.1
    Wh, bh = rn(g, 3, 256) / 8, rn(g, 3) * 0.1
    return Chain([(Dense(W0, b0, L.ACT_RELU, 256, 0, 8, 256), None), (Dense(W1, b1, L.ACT_RELU, 256), None),
                  (Dense(W2, b2, L.ACT_RELU, 256), None), (None, Head(Wh, bh))], k_init=256, k_aux=8).pack()


def sdf_chain(g):
    from nero_amd.chain import Chain
    from nero_amd.sdf import sdf_entries, LD_PE
    shapes = [(256, 39), (256, 256), (256, 256), (217, 256), (256, 256), (256, 256), (256, 256), (256, 256), (257, 256)]
    eff = [(rn(g, o, k) * (1.2 / math.sqrt(k)), rn(g, o) * 0.05) for o, k in shapes]
    return Chain(sdf_entries(eff), k_init=LD_PE, k_aux=LD_PE).pack()


def nerf_head_chain(g):
    from nero_amd import _lib as L
    from nero_amd.chain import Chain, Dense, Head
    W0, b0 = rn(g, 256, 256) / 16, rn(g, 256) * 0.1
    W1, b1 = rn(g, 128, 283) / 16, rn(g, 128) * 0.1
    Wh, bh = rn(g, 3, 128) / 8, rn(g, 3) * 0.1
    return Chain([(Dense(W0, b0, L.ACT_NONE, 256), None), (Dense(W1, b1, L.ACT_RELU, 256, 0, 27, 256), None), (None, Head(Wh, bh))],
                 k_init=256, k_aux=32).pack()


# ---- one launch of each pass, with guarded workspaces, -> the outputs a later kernel reads ---------------------------------------------------
def run_forward(ch, init, aux, n):
    with guarded() as gd:
        o = ch.forward(init, aux, n, save=True)
        torch.cuda.synchronize()
        gd.check()
    out = {}
    for i, s in enumerate(o['saves']):
        if s is not None:
            out[f'save{i}'] = s[:n].clone()
    for i, m in enumerate(o['masks']):
        if m is not None:
            out[f'mask{i}'] = m[:n].clone()
    for i, h in o['heads'].items():
        out[f'head{i}'] = h[:n, :ch.entries[i][1].n_head].clone()
    return o, out


def run_backward(ch, fwd, n, accumulate=None, **kw):
    """accumulate: the [row_pad(n), k_init] content d_init is accumulated ONTO (a fresh guarded copy per launch)"""
    rp = (n + 63) // 64 * 64
    with guarded() as gd:
        if accumulate is not None:
            dview, dfull = guarded_rows(rp, ch.k_init, accumulate)
            kw = dict(kw, dinit_out=dview, accumulate_dinit=True)
        b = ch.backward(fwd, n, **kw)
        torch.cuda.synchronize()
        gd.check()
        if accumulate is not None:
            assert bool((dfull[rp:] == SENT_F).all()), 'sentinel rows of d_init written'
    out = {f'delta{i}': d[:n].clone() for i, d in b['deltas'].items()}
    if b['d_init'] is not None:
        out['d_init'] = b['d_init'][:n].clone()
    if b['d_aux'] is not None:
        out['d_aux'] = b['d_aux'][:n].clone()
    return out


def run_tangent(ch, fwd, ehat, n, n_layers):
    """the tangent chain of nero_amd.sdf.SDFField.backward (injections left to the reverse kernel): adot of layers 0 .. n_layers - 1"""
    from nero_amd import _lib as L
    from nero_amd.chain import _r16, _tiles
    rp = (n + 63) // 64 * 64
    tc = L.TanChain()
    tc.init, tc.ld_init, tc.k_init = ehat.data_ptr(), ehat.stride(0), ch.k_init
    tc.aux, tc.ld_aux, tc.k_aux = ehat.data_ptr(), ehat.stride(0), ch.k_aux
    tc.n_layers, tc.aux_wide, tc.gemm_mode = n_layers, 0, L.GEMM_F16X3
    tc.macs_per_row = float(sum(ch.entries[l][0].n_out * (ch.entries[l][0].k_main + ch.entries[l][0].k_aux) for l in range(n_layers)))
    bufs = [guarded_rows(rp, L.HID) for _ in range(n_layers)]
    for l in range(n_layers):
        d, p, tl = ch.entries[l][0], ch._packed[l], tc.layer[l]
        tl.w_main, tl.w_aux = L.ptr(p.get('hfm')), L.ptr(p.get('hfa'))
        tl.a_saved, tl.gbar, tl.adot, tl.inj = fwd['saves'][l].data_ptr(), None, bufs[l][0].data_ptr(), None
        tl.k_main, tl.k_aux, tl.n_tiles = _r16(d.k_main), (_r16(d.k_aux) if d.k_aux else 0), _tiles(d.n_out)
    L.check(L.lib.nero_mlp_tangent(C.byref(tc), n, L.stream_ptr()))
    torch.cuda.synchronize()
    for view, full in bufs:
        assert bool((full[rp:] == SENT_F).all()), 'sentinel rows of adot written'
    return [view for view, _ in bufs], {f'adot{l}': bufs[l][0][:n].clone() for l in range(n_layers)}


def against_lockstep(paired, mask, launch):
    """launch() under the lock-step kernels once, under the paired kernels (whatever the launch size) twice: all three equal"""
    paired(0)
    ref = launch()
    paired(8 | mask)
    for k in range(2):
        cur = launch()
        assert cur.keys() == ref.keys()
        for name in ref:
            same(cur[name], ref[name], (name, 'run', k))
    paired(0)


# ---- tests -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ROWS)
def test_predictor_forward_and_mask_only_reverse(paired, n):
    g = torch.Generator(device='cuda').manual_seed(100 + n)
    ch = predictor_chain(g)
    rp = (n + 63) // 64 * 64
    init, aux = rn(g, rp, 256), rn(g, rp, 8)
    against_lockstep(paired, 1, lambda: run_forward(ch, init, aux, n)[1])
    paired(0)
    fwd, _ = run_forward(ch, init, aux, n)
    dyh = rn(g, rp, 4) * 1e-2
    against_lockstep(paired, 4, lambda: run_backward(ch, fwd, n, dy=None, head_dys={3: dyh}, need_dinit=True, need_daux=True))
    onto = rn(g, rp, 256)
    against_lockstep(paired, 4, lambda: run_backward(ch, fwd, n, accumulate=onto, dy=None, head_dys={3: dyh}, need_dinit=True, need_daux=True))


@pytest.mark.parametrize('n', ROWS)
def test_sdf_shaped_forward_tangent_and_reverse_with_injections(paired, n):
    from nero_amd.sdf import LD_PE
    g = torch.Generator(device='cuda').manual_seed(200 + n)
    ch = sdf_chain(g)
    rp = (n + 63) // 64 * 64
    last = len(ch.entries) - 1
    pe = rn(g, rp, LD_PE)
    pe[:, 39:] = 0
    against_lockstep(paired, 1, lambda: run_forward(ch, pe, pe, n)[1])
    paired(0)
    fwd, _ = run_forward(ch, pe, pe, n)
    ehat = rn(g, rp, LD_PE) * 0.1
    ehat[:, 39:] = 0
    against_lockstep(paired, 2, lambda: run_tangent(ch, fwd, ehat, n, last)[1])
    paired(0)
    adot, _ = run_tangent(ch, fwd, ehat, n, last)
    gbar = [rn(g, rp, 256) * 1e-2 for _ in range(last)]
    injs = {l: (gbar[l], adot[l]) for l in range(last)}
    d_feat, d_sdf4 = rn(g, rp, 256) * 1e-2, rn(g, rp, 4) * 1e-2
    against_lockstep(paired, 4, lambda: run_backward(ch, fwd, n, dy=d_feat, head_dys={last: d_sdf4}, injs=injs))
    ones = torch.zeros(rp, 4, device='cuda')
    ones[:, 0] = 1.0
    against_lockstep(paired, 4, lambda: run_backward(ch, fwd, n, dy=None, head_dys={last: ones}, need_dinit=True, need_daux=True,
                                                     skip_last_dense=True))


@pytest.mark.parametrize('n', ROWS)
def test_nerf_head_chain_forward_and_reverse(paired, n):
    g = torch.Generator(device='cuda').manual_seed(300 + n)
    ch = nerf_head_chain(g)
    rp = (n + 63) // 64 * 64
    init, aux = rn(g, rp, 256), rn(g, rp, 32)
    against_lockstep(paired, 1, lambda: run_forward(ch, init, aux, n)[1])
    paired(0)
    fwd, _ = run_forward(ch, init, aux, n)
    dyh = rn(g, rp, 4) * 1e-2
    against_lockstep(paired, 4, lambda: run_backward(ch, fwd, n, dy=None, head_dys={2: dyh}, need_dinit=True, need_daux=True))
