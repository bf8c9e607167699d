"""The environment-light export (nero_amd/envlight.py, nero_amd/csrc/envlight.hip) on one MI355X: HIP events around `inner` back-to-back runs of
each phase on a seeded network, a warm-up of every shape, the median over --reps, a device synchronise before any clock is read.  Writes one
JSON document (--out) and prints it.

    python scripts/bench_envlight.py [--reps 10] [--out profiles/bench_envlight.json]

Sizes: 512 x 1024 (the command line's default) and 2048 x 4096, 'direction' light, chunks of nero_amd.envlight.DEFAULT_CHUNK pixels.  For each:
  encode        nero_env_encode over all chunks (writes 288 bytes of encoding per pixel)
  chain         the outer_light chain forward over all chunks, on one chunk's encodings (72 -> 256 -> 256 -> 256 -> 3: 150 272 MACs per pixel)
  finish_rgbe   nero_env_finish over all chunks and nero_env_rgbe over the whole map
  whole         NeROMaterialRenderer.env_light(gamma=False) and rgbe_encode: the call a user makes, allocation included
  torch_gpu     the reference's formulation in plain torch on the same GPU: the host-built grid moved to the device, batches of 8192 through
                the IDE (oracle.nero_oracle.ide) and four F.linear layers on the effective weights, exp and the concatenation; no RGBE
`check` holds the largest relative difference between the two routes on the 512 x 1024 map.  Times are of calls (HIP events), not a profiler's
kernel times; anything not measured here is absent from the document, not estimated."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(512, 1024), (2048, 4096)]
MACS_PER_PIXEL = 72 * 256 + 256 * 256 + 256 * 256 + 256 * 3


def timed(fn, reps, inner, warmup=2):
    """-> list of milliseconds per call (HIP events around `inner` calls, one synchronise per repetition)"""
    out = []
    for it in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(a.elapsed_time(b) / inner)
    return out


def stats(ms, **extra):
    med = statistics.median(ms)
    return dict({'ms': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4)}, **extra)


def torch_formulation(P, h, w, exp_max, dev):
    """network/field.py:1020-1047 in plain torch on the device (synthetic axes, gamma=False)"""
    from oracle import nero_oracle as O
    azs = torch.linspace(1.0, 0.0, w) * np.pi * 2 - np.pi / 2
    els = torch.linspace(1.0, -1.0, h) * np.pi / 2
    els, azs = torch.meshgrid(els, azs, indexing='ij')
    xyz = torch.stack([torch.cos(els) * torch.sin(azs), torch.sin(els), torch.cos(els) * torch.cos(azs)], -1).reshape(h * w, 3).to(dev)
    out = []
    with torch.no_grad():
        for ri in range(0, h * w, 8192):
            out.append(O.predictor(P, 'shader_network.outer_light', O.ide(xyz[ri:ri + 8192], 0.0), O._exp_act(exp_max)))
    return torch.cat(out, 0).reshape(h, w, 3)


def bench_size(net, P, h, w, reps, dev):
    from nero_amd import _lib as L
    from nero_amd import envlight as E
    from nero_amd.chain import row_pad
    lib = E._lib
    with torch.no_grad():
        _, _, K = net._kernels()
    chain, exp_max = K.outer_light, net.shader_network.cfg['light_exp_max']
    n_px = h * w
    chunk = min(E.DEFAULT_CHUNK, n_px)
    firsts = list(range(0, n_px, chunk))
    inner = max(1, (1 << 21) // n_px)
    X = torch.empty((row_pad(chunk), 72), dtype=torch.float32, device=dev)
    rgb = torch.empty((n_px, 3), dtype=torch.float32, device=dev)
    rgbe = torch.empty((n_px, 4), dtype=torch.uint8, device=dev)

    def encode():
        for f in firsts:
            L.check(lib.nero_env_encode(h, w, f, min(chunk, n_px - f), 0, 0, 0.0, L.ptr(X), None, L.stream_ptr()))
    encode()
    raw = [None]

    def chain_fwd():
        for f in firsts:
            raw[0] = chain.forward(X, None, min(chunk, n_px - f), save=False)['heads'][3]
    chain_fwd()

    def finish_rgbe():
        for f in firsts:
            n = min(chunk, n_px - f)
            L.check(lib.nero_env_finish(L.ptr(raw[0]), n, float(exp_max), 0, L.ptr(rgb[f:f + n]), L.stream_ptr()))
        L.check(lib.nero_env_rgbe(L.ptr(rgb), n_px, L.ptr(rgbe), L.stream_ptr()))

    def whole():
        E.rgbe_encode(net.env_light(h, w, gamma=False))
    res = {'h': h, 'w': w, 'pixels': n_px, 'chunk': chunk, 'chunks': len(firsts), 'reps': reps, 'inner': inner}
    ms = timed(encode, reps, inner)
    res['encode'] = stats(ms, bytes_written=288 * n_px, bytes_per_s=round(288 * n_px / (statistics.median(ms) * 1e-3), 0))
    ms = timed(chain_fwd, reps, inner)
    res['chain'] = stats(ms, macs=MACS_PER_PIXEL * n_px, flop_per_s=round(2 * MACS_PER_PIXEL * n_px / (statistics.median(ms) * 1e-3), 0))
    res['finish_rgbe'] = stats(timed(finish_rgbe, reps, inner))
    res['whole'] = stats(timed(whole, reps, inner))
    res['torch_gpu'] = stats(timed(lambda: torch_formulation(P, h, w, exp_max, dev), max(3, reps // 3), 1, warmup=1))
    res['torch_gpu_over_whole'] = round(res['torch_gpu']['ms'] / res['whole']['ms'], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'bench_envlight.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_envlight.py measures on a GPU; none is visible')
    dev = torch.device('cuda:0')
    from nero_amd.renderer import NeROMaterialRenderer
    from nero_amd.synthetic import icosphere, perturb_state
    from oracle import nero_oracle as O
    torch.manual_seed(6033)
    net = NeROMaterialRenderer({'shader_cfg': {'human_lights': False}, 'database_name': 'syn/bench'}, is_train=False, mesh=icosphere(1, 0.5))
    perturb_state(net, None)
    net = net.to(dev).eval()
    P = O.effective_params({k: v.detach() for k, v in net.state_dict().items()})
    with torch.no_grad():
        ours = net.env_light(512, 1024, gamma=False)
        theirs = torch_formulation(P, 512, 1024, net.shader_network.cfg['light_exp_max'], dev)
    check = float(((ours - theirs).abs() / theirs).max())
    out = {'metric': 'env_light_export', 'device': torch.cuda.get_device_name(0), 'timing': 'HIP events around `inner` runs of a phase over all chunks',
           'check': {'size': [512, 1024], 'max_rel_difference_hip_vs_torch': check},
           'sizes': [bench_size(net, P, h, w, args.reps, dev) for h, w in SIZES]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
