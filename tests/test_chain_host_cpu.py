"""The C++ twin of nero_amd/chain.py::Chain (the planner of nero_amd/csrc/chain_host.h) against its Python original, without a GPU:
tests/chain_host_main.cpp is built with the host compiler under ASan + UBSan -- the header holds no device code -- and run on dry arenas;
its pack sizes, pack jobs and chain offsets must be the Python twin's, its arena peaks the ones the header gave before the planner was
split from its kernels (tests/golden/chain_host_peaks.txt)."""
import os

import torch

from tests.helpers import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 63, 64, 65, 4097)                       # each side of a 64-row tile edge, and many tiles
NAMES = ('predictor', 'predictor_no_aux', 'feats')


def _program(tmp_path):
    """stdout of the program, as {first word: [the other words of each such line]}"""
    stdout = run_host_program(tmp_path, 'chain_host_main.cpp', extra=('-I' + os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include'),))
    out = {}
    for ln in stdout.splitlines():
        out.setdefault(ln.split()[0], []).append(ln.split()[1:])
    return out


def _twins():
    """{name: (Chain on CPU tensors, {data_ptr of an entry's weight or bias: entry})}: the three chains of the program"""
    from nero_amd import _lib as L
    from nero_amd.chain import Chain, Dense
    from nero_amd.shape_step import predictor_entries
    lin = lambda n_out, k: (torch.zeros(n_out, k), torch.zeros(n_out))
    pred = lambda k0, n_head: [lin(256, k0), lin(256, 256), lin(256, 256), lin(n_head, 256)]
    f = [lin(256, 51 if i == 0 else (307 if i == 4 else 256)) for i in range(8)]          # MaterialKernels.feats: skip into layer 4
    feats = [(Dense(W, b, L.ACT_NONE if i == 7 else L.ACT_RELU, *((256, 0, 51, 256) if i == 4 else (51 if i == 0 else 256,))), None)
             for i, (W, b) in enumerate(f)]
    chains = {'predictor': Chain(predictor_entries(pred(259, 3), 256, 3), k_init=256, k_aux=8, device='cpu'),
              'predictor_no_aux': Chain(predictor_entries(pred(123, 3), 123), k_init=128, device='cpu'),
              'feats': Chain(feats, k_init=56, k_aux=56, aux_wide=True, device='cpu')}
    out = {}
    for name, c in chains.items():
        entry = {}
        for i, (d, h) in enumerate(c.entries):
            for t in ((d.W, d.b) if d is not None else ()) + ((h.W, h.b) if h is not None else ()):
                entry[t.data_ptr()] = i
        out[name] = (c, entry)
    return out


def test_the_planner_is_its_python_twin_under_the_sanitizer(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import chain
    prog = _program(tmp_path)                       # exit 0 and a silent stderr: no sanitizer report, no stub reached
    assert [w[0] for w in prog['chain']] == list(NAMES)
    assert [(w[0], int(w[1])) for w in prog['peak']] == [(n, r) for n in NAMES for r in ROWS]
    twins = _twins()
    before = dict(chain.GEMM_MODE)
    chain.set_gemm_mode('f16x3')                    # the one arithmetic the C-level drivers pack
    try:
        for w in prog['chain']:
            name = w[0]
            c, entry = twins[name]
            assert int(w[2]) == c.pack_floats(), name
            # the jobs per entry, as sets: the twins order the images of an entry differently, so the image address is left out
            mine, theirs = {}, {}
            for j, _ in c.pack(run=False):
                mine.setdefault(entry[j.W], set()).add((j.kind, j.nrows, j.ld, j.col0, j.ncols, j.transpose, j.kpad, j.nt_count, float(j.scale)))
            for j in prog['job']:
                if j[0] == name:
                    theirs.setdefault(int(j[1]), set()).add(tuple(int(x) for x in j[2:10]) + (float(j[10]),))
            assert sum(len(s) for s in theirs.values()) == int(w[4]) == sum(len(s) for s in mine.values()), name     # no job twice
            assert theirs == mine, name
        sizes = [(twins[n][0].pack_floats() + 63) // 64 * 64 for n in NAMES]
    finally:
        chain.GEMM_MODE.update(before)
    # pack_chains / carve_chains: every chain at a 64-float boundary, in order
    assert [int(x) for x in prog['offsets'][0]] == [sum(sizes[:i]) for i in range(len(sizes))]
    assert int(prog['total'][0][0]) == sum(sizes) and int(prog['total'][0][2]) == len(prog['job'])
    # arena peaks of forward(save) + backward(d_init, d_aux): what the header gave before this program could be built without hipcc
    golden = [ln.split()[1:] for ln in open(os.path.join(ROOT, 'tests', 'golden', 'chain_host_peaks.txt')) if ln.startswith('peak')]
    assert len(golden) == len(NAMES) * len(ROWS) and prog['peak'] == golden
    # (the first chain by hand, at one 64-row tile: a head, three saves with their ReLU masks; then d_init, d_aux and three deltas)
    assert int(golden[0][2]) == 64 * 4 * (4 + 3 * 256 + 3 * 8) + 64 * 4 * (256 + 8 + 3 * 256) == 467968
