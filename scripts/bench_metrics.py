"""The validation metrics (nero_amd/metrics.py, nero_amd/csrc/image_metrics.hip) on one MI355X: HIP events around `--inner` back-to-back calls on
seeded inputs, a warm-up, the median over --reps, a device synchronise before any clock is read.  Writes one JSON document (--out) and prints it.

    python scripts/bench_metrics.py [--reps 20] [--inner 20] [--out profiles/bench_metrics.json]

Sizes: one 800 x 800 x 3 view (the synthetic scenes), one 1024 x 768 x 3 view, a batch of 8 views of 800 x 800 x 3.  For each:
  quantize          nero_img_quantize alone on the float images of the pair (reads 4 bytes and writes 1 per value)
  metrics           nero_img_metrics alone on the 8-bit pair (needs 2 h w C bytes per image: each byte of both images once)
  shape_metrics     the whole ShapeRenderMetrics call, write_vis=False, per view, with its one device-to-host copy of the two numbers
  host_reference    the reference's formulation on the host cores: the two float images copied to the host, color_map_backward, the float32
                    PSNR, and SSIM by scipy.ndimage.uniform_filter in float64 (tests/metrics_ref.py), per view
  torch_gpu         the same formulation in plain torch on the GPU: float64 avg_pool2d of x, y, x^2, y^2, x y
bytes_per_s is the bytes the algorithm needs over the measured time of a call (HIP events around the call, not a profiler's kernel time), beside
the HBM rates of the MI355X: 8.0e12 bytes/s in the data sheet, 6.3e12 measured for a float4 copy.  Anything not measured here is absent from the
document, not estimated."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
SIZES = [('800x800x3', 1, 800, 800, 3), ('1024x768x3', 1, 768, 1024, 3), ('8x800x800x3', 8, 800, 800, 3)]


def timed(fn, reps, inner, warmup=3):
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


def host_timed(fn, reps, warmup=1):
    """-> list of milliseconds of a host function that ends synchronised"""
    out = []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(ms, nbytes=None):
    med = statistics.median(ms)
    out = {'ms': round(med, 5), 'ms_min': round(min(ms), 5), 'ms_max': round(max(ms), 5)}
    if nbytes is not None:
        rate = nbytes / (med * 1e-3)
        out.update({'bytes': int(nbytes), 'bytes_per_s': round(rate, 0), 'share_of_hbm_spec': round(rate / HBM_SPEC, 4),
                    'share_of_hbm_float4_copy': round(rate / HBM_COPY, 4)})
    return out


def torch_gpu_formulation(gt, pr):
    """float images [h, w, 3] on the device -> (psnr, ssim) device scalars: the reference's formulation in plain torch"""
    q = lambda x: torch.clamp(x * 255, 0, 255).to(torch.uint8)
    g, p = q(gt), q(pr)
    a, b = g.reshape(-1, 3).float(), p.reshape(-1, 3).float()
    psnr = 10 * torch.log10(255 * 255 / ((a - b) ** 2).mean(0).mean())
    x, y = g.permute(2, 0, 1)[None].double(), p.permute(2, 0, 1)[None].double()
    f = lambda t: torch.nn.functional.avg_pool2d(t, 11, stride=1)
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    n = 121 / 120
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return psnr, s.mean()


def bench_size(name, B, h, w, c, reps, inner, dev):
    from nero_amd import _lib as L
    from nero_amd import metrics as M
    from tests import metrics_ref as R
    g = torch.Generator().manual_seed(B * h + w)
    gt = torch.rand((B, h, w, c), generator=g).to(dev)
    pr = (gt + 0.05 * torch.randn((B, h, w, c), generator=g).to(dev)).contiguous()
    n = gt.numel()
    qg, qp = torch.empty(gt.shape, dtype=torch.uint8, device=dev), torch.empty(gt.shape, dtype=torch.uint8, device=dev)
    lib = M._lib

    def quantize():
        L.check(lib.nero_img_quantize(L.ptr(gt), n, L.ptr(qg), L.stream_ptr()))
        L.check(lib.nero_img_quantize(L.ptr(pr), n, L.ptr(qp), L.stream_ptr()))
    ws = torch.empty(int(lib.nero_img_metrics_workspace_bytes(B, h, w, c)), dtype=torch.uint8, device=dev)
    out = torch.empty((B, 2), dtype=torch.float64, device=dev)
    metrics = lambda: L.check(lib.nero_img_metrics(L.ptr(qg), L.ptr(qp), B, h, w, c, L.ptr(ws), None, None, L.ptr(out), L.stream_ptr()))
    res = {'size': name, 'B': B, 'h': h, 'w': w, 'C': c, 'reps': reps, 'inner': inner}
    res['quantize'] = stats(timed(quantize, reps, inner), 2 * 5 * n)
    res['quantize']['note'] = 'both images of the pair: two launches'
    res['metrics'] = stats(timed(metrics, reps, inner), 2 * n)
    res['metrics']['workspace_bytes'] = ws.numel()

    shape_metric = M.ShapeRenderMetrics({'write_vis': False})
    views = [{'gt_rgb': gt[b], 'ray_rgb': pr[b]} for b in range(B)]
    def whole():
        for b, v in enumerate(views):
            shape_metric(v, {}, 0, data_index=b, model_name='bench')
    ms = host_timed(whole, reps, warmup=2)
    res['shape_metrics_per_view'] = stats([m / B for m in ms])
    res['shape_metrics_per_view']['note'] = 'host clock: two quantise launches, the metrics, one device-to-host copy of two float64'

    def host_reference():
        for b in range(B):
            a, p = R.color_map_backward(gt[b].cpu().numpy()), R.color_map_backward(pr[b].cpu().numpy())
            R.psnr_ref32(a, p)
            R.ssim_ref(a, p)
    ms = host_timed(host_reference, max(3, reps // 4))
    res['host_reference_per_view'] = stats([m / B for m in ms])
    res['host_reference_per_view']['threads'] = torch.get_num_threads()

    def torch_gpu():
        for b in range(B):
            torch_gpu_formulation(gt[b], pr[b])
    res['torch_gpu_per_view'] = stats([m / B for m in timed(torch_gpu, reps, 1)])

    # the three routes on the same view: what they computed
    ours = out.cpu().numpy()[0]
    a, p = R.color_map_backward(gt[0].cpu().numpy()), R.color_map_backward(pr[0].cpu().numpy())
    tp, ts = torch_gpu_formulation(gt[0], pr[0])
    res['view0'] = {'psnr': float(ours[0]), 'ssim': float(ours[1]), 'psnr_exact_host': R.psnr_exact(a, p), 'psnr_float32_host': float(R.psnr_ref32(a, p)),
                    'ssim_host': R.ssim_ref(a, p)[0], 'psnr_torch_gpu': float(tp), 'ssim_torch_gpu': float(ts)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'bench_metrics.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_metrics.py measures on a GPU; none is visible')
    dev = torch.device('cuda:0')
    out = {'metric': 'validation_metrics', 'device': torch.cuda.get_device_name(0), 'hbm_bytes_per_s_spec': HBM_SPEC,
           'hbm_bytes_per_s_float4_copy': HBM_COPY, 'timing': 'HIP events around `inner` calls; host clock where noted',
           'sizes': [bench_size(*s, args.reps, args.inner, dev) for s in SIZES]}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
