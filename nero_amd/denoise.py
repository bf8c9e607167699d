"""Edge-aware denoising of the relighter's pictures on the GPU (include/nero_hip_denoise.h, nero_amd/csrc/denoise.hip): a
single-frame edge-avoiding a-trous wavelet filter steered by normals, tangent-plane distance, optional extra guide channels and a variance
estimated from the picture itself.  Nothing temporal, no per-sample variance.

It works on an h x w image at the resolution that was traced -- every pixel one surface or none -- on two records per pixel that this module
packs in torch: guide [n,8] = (normal, valid, position, 0), or [n,12] with four more guide channels, and signal [n,4] = (rgb, variance).
Relighter.render(denoise=...) filters its diffuse, specular and indirect signals through denoise() below."""
import torch

from . import _lib as L

_lib = L.lib
DEFAULTS = {'iterations': 5, 'sigma_l': 4.0, 'normal_pow2': 6, 'sigma_p': None, 'sigma_g': 0.1}      # denoise()'s, and render(denoise=True)'s
MAX_ITERATIONS = 21                                               # step = 2^(iterations - 1) <= 2^20


def pack_guides(pos, normal, valid, extra=None):
    """pos [n,3], normal [n,3], valid [n] (bool or 0 / 1), extra [n,4] or None -> guide [n,8] or [n,12] float32, contiguous.  The record of
    an invalid pixel is all zeros: whatever its position and normal held (NaN, infinity) never meets arithmetic."""
    n = pos.shape[0]
    v = valid.reshape(n) != 0
    cols = [normal.reshape(n, 3).float(), v.float()[:, None], pos.reshape(n, 3).float(), torch.zeros(n, 1, device=pos.device)]
    if extra is not None:
        cols.append(extra.reshape(n, 4).float())
    g = torch.cat(cols, -1)
    return torch.where(v[:, None], g, torch.zeros_like(g)).contiguous()


def pack_signal(rgb, var=None):
    """rgb [n,3], var [n] or None (zeros) -> signal [n,4] float32, contiguous"""
    n = rgb.shape[0]
    v = torch.zeros(n, 1, device=rgb.device) if var is None else var.reshape(n, 1).float()
    return torch.cat([rgb.reshape(n, 3).float(), v], -1).contiguous()


def _records(guide, sig, h, w):
    guide, sig = guide.float().contiguous(), sig.float().contiguous()
    n = int(h) * int(w)
    if guide.ndim != 2 or guide.shape[1] not in (8, 12) or guide.shape[0] != n or tuple(sig.shape) != (n, 4):
        raise ValueError(f'guide [{n},8] or [{n},12] and signal [{n},4] expected for a {h} x {w} image, got {tuple(guide.shape)} and {tuple(sig.shape)}')
    return guide, sig, guide.shape[1] - 8


def estimate_variance(guide, sig, h, w, normal_pow2=6, sigma_p=0.05, sigma_g=0.1, out=None):
    """nero_denoise_variance: the guide-weighted variance of the luminance over each valid pixel's 7 x 7 window -> signal [n,4] with it in
    the fourth column, rgb copied through (a new tensor, or `out`, which must not be `sig`)"""
    guide, sig, G = _records(guide, sig, h, w)
    out = torch.empty_like(sig) if out is None else out
    with torch.cuda.device(sig.device):
        L.check(_lib.nero_denoise_variance(L.ptr(guide), G, L.ptr(sig), int(h), int(w), int(normal_pow2), float(sigma_p), float(sigma_g),
                                           L.ptr(out), L.stream_ptr()))
    return out


def atrous_pass(guide, sig, h, w, step, normal_pow2=6, sigma_l=4.0, sigma_p=0.05, sigma_g=0.1, out=None):
    """nero_denoise_atrous: one iteration at stride `step` -> signal [n,4] (a new tensor, or `out`, which must not be `sig`)"""
    guide, sig, G = _records(guide, sig, h, w)
    out = torch.empty_like(sig) if out is None else out
    with torch.cuda.device(sig.device):
        L.check(_lib.nero_denoise_atrous(L.ptr(guide), G, L.ptr(sig), int(h), int(w), int(step), int(normal_pow2), float(sigma_l),
                                         float(sigma_p), float(sigma_g), L.ptr(out), L.stream_ptr()))
    return out


def denoise_records(guide, sig, h, w, iterations=5, sigma_l=4.0, normal_pow2=6, sigma_p=0.05, sigma_g=0.1):
    """the variance pass and `iterations` a-trous passes at strides 1, 2, 4, ... over packed records, between two buffers -> signal [n,4]"""
    iterations = int(iterations)
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f'iterations {iterations}: 0 to {MAX_ITERATIONS}')
    a = estimate_variance(guide, sig, h, w, normal_pow2, sigma_p, sigma_g)
    b = torch.empty_like(a)
    for it in range(iterations):
        atrous_pass(guide, a, h, w, 1 << it, normal_pow2, sigma_l, sigma_p, sigma_g, out=b)
        a, b = b, a
    return a


def denoise(rgb, pos, normal, valid, h, w, extra=None, iterations=5, sigma_l=4.0, normal_pow2=6, sigma_p=0.05, sigma_g=0.1):
    """rgb, pos, normal [h w,3], valid [h w], extra [h w,4] or None (CUDA tensors, row-major over the image) -> (filtered rgb [h w,3], the
    final variance [h w]).  iterations: a-trous passes, the stride doubling from 1; sigma_l: how many standard deviations of luminance a tap
    may differ by; normal_pow2 = k: the normal weight is max(0, n . n')^(2^k); sigma_p: the tangent-plane distance, in the units of pos, at
    which a tap's weight falls to 1 / e; sigma_g: the same for the distance in the extra channels.  Invalid pixels come back unchanged."""
    guide = pack_guides(pos, normal, valid, extra)
    out = denoise_records(guide, pack_signal(rgb), h, w, iterations, sigma_l, normal_pow2, sigma_p, sigma_g)
    return out[:, :3].contiguous(), out[:, 3].contiguous()


def options(denoise_arg, sigma_p_default):
    """render(denoise=...)'s argument -> None (off) or the keyword arguments of denoise(): True takes DEFAULTS, a dict overrides them; a
    sigma_p of None becomes sigma_p_default"""
    if denoise_arg is None or denoise_arg is False:
        return None
    opts = dict(DEFAULTS)
    if denoise_arg is not True:
        unknown = set(denoise_arg) - set(DEFAULTS)
        if unknown:
            raise ValueError(f'denoise: unknown parameters {sorted(unknown)}; known: {sorted(DEFAULTS)}')
        opts.update(denoise_arg)
    if opts['sigma_p'] is None:
        opts['sigma_p'] = sigma_p_default
    return opts
