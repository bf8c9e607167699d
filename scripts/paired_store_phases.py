"""Where the row stores of the paired chain kernels (nero_amd/csrc/mlp_f16p.hip) cost their time: per-phase shader-clock cycles of
fwd_p_kernel per (64-row tile, layer) with the step's chain shapes -- the SDF network with saves, a material predictor with saves, sign
words and a head -- once as the step runs them and once with the save pointers nulled, plus the wall time per launch of the forward,
tangent and reverse chains.  Run on the GPU with a library whose mlp_f16p.hip was built with -DF16_PHASE_TIMING:
    NERO_HIP_LIB=build/variants/libp_phase.so python scripts/paired_store_phases.py [rows]
(without the instrumentation only the wall times are printed)."""
import ctypes as C
import math
import sys
import time

import torch

sys.path.insert(0, '.')
from nero_amd import _lib as L            # noqa: E402
from nero_amd import chain as CH          # noqa: E402
from nero_amd.chain import Chain, Dense, Head, row_pad, _r16, _tiles      # noqa: E402
from nero_amd.sdf import sdf_entries, LD_PE                             # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
REP = 5
rp = row_pad(N)
tiles = rp // 64
g = torch.Generator(device='cuda').manual_seed(0)
rn = lambda *s: torch.randn(*s, device='cuda', generator=g)
CH.f16_paired(8 | 7)
has_ph = hasattr(L.lib, 'nero_debug_phases_p')
buf = (C.c_ulonglong * 16)()
NAMES = ('init', 'pre-gemm', 'gemm', 'values', 'stores+masks', 'commit', '-', 'residence')


def phases():
    if not has_ph:
        return None
    L.lib.nero_debug_phases_p(buf, 1)
    return [int(v) for v in buf[:8]]


def timeit(f):
    f()
    torch.cuda.synchronize()
    phases()
    t = time.time()
    for _ in range(REP):
        f()
    torch.cuda.synchronize()
    return (time.time() - t) / REP, phases()


def report(name, t, ph, n_layers):
    print(f'{name:34s} {t * 1e3:8.3f} ms   {t * 1e6 / (tiles / 256 * n_layers):6.2f} us per layer-tile per CU')
    if ph:
        per = REP * tiles * n_layers
        print('      ' + '  '.join(f'{n}={p / per:.0f}' for n, p in zip(NAMES, ph) if n != '-') + '   (cycles of wave 0 per layer-tile)')


def sdf_chain():
    shapes = [(256, 39), (256, 256), (256, 256), (217, 256), (256, 256), (256, 256), (256, 256), (256, 256), (257, 256)]
    eff = [(rn(o, k) * (1.2 / math.sqrt(k)), rn(o) * 0.05) for o, k in shapes]
    return Chain(sdf_entries(eff), k_init=LD_PE, k_aux=LD_PE).pack()


def predictor_chain():
    Ws = [(rn(256, 264) / 16, rn(256) * 0.1)] + [(rn(256, 256) / 16, rn(256) * 0.1) for _ in range(3)]
    ent = [(Dense(Ws[0][0], Ws[0][1], L.ACT_RELU, 256, 0, 8, 256), None)] + [(Dense(W, b, L.ACT_RELU, 256), None) for W, b in Ws[1:]]
    return Chain(ent + [(None, Head(rn(3, 256) / 8, rn(3) * 0.1))], k_init=256, k_aux=8).pack()


print(f'rows {N}, {tiles} tiles, phase counters: {"yes" if has_ph else "no"}')
sdf = sdf_chain()
pe = rn(rp, LD_PE)
pe[:, 39:] = 0
for save in (True, False):
    t, ph = timeit(lambda: sdf.forward(pe, pe, N, save=save))
    report(f'fwd sdf        save={int(save)}', t, ph, 9)
pred = predictor_chain()
x, aux = rn(rp, 256), rn(rp, 8)
for save in (True, False):
    t, ph = timeit(lambda: pred.forward(x, aux, N, save=save))
    report(f'fwd predictor  save={int(save)}', t, ph, 4)

# tangent and reverse of the same chains: wall time per launch (their kernels carry no phase counters)
fwd = sdf.forward(pe, pe, N, save=True)
last = len(sdf.entries) - 1
ehat = rn(rp, LD_PE) * 0.1
ehat[:, 39:] = 0
tc = L.TanChain()
tc.init, tc.ld_init, tc.k_init = ehat.data_ptr(), LD_PE, LD_PE
tc.aux, tc.ld_aux, tc.k_aux = ehat.data_ptr(), LD_PE, LD_PE
tc.n_layers, tc.aux_wide, tc.gemm_mode = last, 0, L.GEMM_F16X3
tbuf = torch.empty((last, rp, L.HID), device='cuda')
for l in range(last):
    d, p, tl = sdf.entries[l][0], sdf._packed[l], tc.layer[l]
    tl.w_main, tl.w_aux = L.ptr(p.get('hfm')), L.ptr(p.get('hfa'))
    tl.a_saved, tl.gbar, tl.adot, tl.inj = fwd['saves'][l].data_ptr(), None, tbuf[l].data_ptr(), None
    tl.k_main, tl.k_aux, tl.n_tiles = _r16(d.k_main), (_r16(d.k_aux) if d.k_aux else 0), _tiles(d.n_out)
t, _ = timeit(lambda: L.check(L.lib.nero_mlp_tangent(C.byref(tc), N, L.stream_ptr())))
report('tan sdf', t, None, last)
gbar = [rn(rp, 256) * 1e-2 for _ in range(last)]
injs = {l: (gbar[l], tbuf[l]) for l in range(last)}
d_feat, d_sdf4 = rn(rp, 256) * 1e-2, rn(rp, 4) * 1e-2
t, _ = timeit(lambda: sdf.backward(fwd, N, dy=d_feat, head_dys={last: d_sdf4}, injs=injs))
report('bwd sdf        +injections', t, None, 9)
pf = pred.forward(x, aux, N, save=True)
dyh = rn(rp, 4) * 1e-2
t, _ = timeit(lambda: pred.backward(pf, N, dy=None, head_dys={4: dyh}, need_dinit=True, need_daux=True))
report('bwd predictor  masks only', t, None, 4)
