"""The learned environment light as lat-long (equirectangular) maps on the device (libnero_hip.so, nero_env_*), and the Radiance .hdr container.

The reference renders the estimated illumination with MCShadingNetwork.env_light(h, w, gamma) and samples it at its 8192 Fibonacci light_pts
with get_env_light() (network/field.py:1020-1059): a host-built direction grid, sph_enc, the outer_light predictor in batches of 8192.  Here
  * latlong_directions: the direction grid, derived on the device from the pixel index (nero_env_encode);
  * render_env_light: encode -> outer_light chain forward (the cached packed kernels of the renderers) -> exp / linear_to_srgb
    (nero_env_finish), in row chunks; the workspace is bounded by the chunk and the result is bit-identical for every chunking;
  * eval_env_light: the same light at given directions (get_env_light);
  * rgbe_encode / rgbe_decode, write_hdr / read_hdr: Radiance RGBE (nero_env_rgbe) and the `#?RADIANCE` file, the input of relight.py --hdr.
Conventions (include/nero_hip.h): the panorama is [h, w, 3] row-major; pixel (row r, column c) looks along az = linspace(1, 0, w)[c] 2 pi - pi / 2,
el = linspace(1, -1, h)[r] pi / 2; d = (cos el cos az, cos el sin az, sin el) for real data (z up), (cos el sin az, sin el, cos el cos az) for
synthetic data (y up).  Row 0 is the pole el = +pi / 2 and the .hdr stores rows top to bottom (-Y h +X w), so the file shows the sky at its top.

One difference from the reference, on purpose: a direction exactly on the z axis -- the synthetic convention's pixel (row (h - 1) / 2, column
3 (w - 1) / 4) when both are integers, e.g. (8, 24) of a 17 x 33 map -- is NaN in the reference (its IDE raises 0 to a complex power); here it
is the finite limit of the encoding, what the neighbouring pixels converge to."""
import numpy as np
import torch

from . import _lib as L
from .chain import row_pad

_lib = L.lib

DEFAULT_CHUNK = 1 << 16     # rows per encode / chain / finish round when chunk is None: 37 MB of encodings + 67 MB of chain activations
MAX_SIZE = 16384
RGBE_MIN = 1e-32            # a pixel whose largest channel is below this is stored as (0, 0, 0, 0)
RGBE_LIMIT = 2.0 ** 127     # ... and the exponent byte holds values below this


def _device(device):
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('the environment light is rendered on the GPU: give a CUDA device')
    return device


def _check_size(h, w):
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f'a panorama of {h} x {w} pixels: both sizes must be in [1, {MAX_SIZE}]')
    return h, w


# ---- kernels --------------------------------------------------------------------------------------------------------------------------------
def latlong_directions(h, w, is_real, device=None):
    """-> float32 [h, w, 3] on the device: the unit direction of every pixel of an h x w lat-long panorama (the grid of env_light,
    network/field.py:1021-1034), derived on the device from the pixel index (nero_env_encode without the encoding)"""
    h, w = _check_size(h, w)
    dev = _device(device)
    with torch.cuda.device(dev):
        dirs = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        L.check(_lib.nero_env_encode(h, w, 0, h * w, int(bool(is_real)), 0, 0.0, None, L.ptr(dirs), L.stream_ptr()))
    return dirs


def _finish(raw, n, exp_max, gamma, out):
    L.check(_lib.nero_env_finish(L.ptr(raw), n, float(exp_max), int(bool(gamma)), L.ptr(out), L.stream_ptr()))


def render_env_light(chain, h, w, is_real, sphere, exp_max, gamma=True, roughness=0.0, chunk=None, device=None):
    """the panorama of one outer_light chain (a packed nero_amd.chain.Chain whose first layer takes 72, with `sphere` 144, columns):
    -> contiguous float32 [h, w, 3] on the device, exp(min(raw, exp_max)), through linear_to_srgb when gamma, never clamped to 1.
    chunk: pixels per round (None: DEFAULT_CHUNK); the encodings and the chain's activations are allocated for one chunk, the output alone
    for h w.  Every pixel's value depends on its index alone: the same bits for every chunk size."""
    h, w = _check_size(h, w)
    dev = _device(device)
    n_px = h * w
    chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f'chunk must be at least 1, got {chunk}')
    chunk = min(chunk, n_px)
    ld = 144 if sphere else 72
    if chain.k_init != ld:
        raise ValueError(f'the outer_light chain takes {chain.k_init} input columns, the encoding has {ld}')
    with torch.cuda.device(dev), torch.no_grad():
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        flat = out.view(n_px, 3)
        X = torch.empty((row_pad(chunk), ld), dtype=torch.float32, device=dev)
        for first in range(0, n_px, chunk):
            n = min(chunk, n_px - first)
            L.check(_lib.nero_env_encode(h, w, first, n, int(bool(is_real)), int(bool(sphere)), float(roughness), L.ptr(X), None, L.stream_ptr()))
            raw = chain.forward(X, None, n, save=False)['heads'][3]
            _finish(raw, n, exp_max, gamma, flat[first:first + n])
    return out


def eval_env_light(chain, dirs, sphere, exp_max, gamma=False, roughness=0.0):
    """the same light at given directions dirs [n, 3] (device tensor) -> float32 [n, 3]: predict_outer_lights_pts (network/field.py:1049-1055)"""
    if not (torch.is_tensor(dirs) and dirs.is_cuda and dirs.dim() == 2 and dirs.shape[1] == 3):
        raise ValueError('eval_env_light: a CUDA tensor [n, 3] of directions is expected')
    dev = dirs.device
    dirs = dirs.detach().to(torch.float32).contiguous()
    n = dirs.shape[0]
    ld = 144 if sphere else 72
    if chain.k_init != ld:
        raise ValueError(f'the outer_light chain takes {chain.k_init} input columns, the encoding has {ld}')
    with torch.cuda.device(dev), torch.no_grad():
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n:
            X = torch.empty((row_pad(n), ld), dtype=torch.float32, device=dev)
            L.check(_lib.nero_env_encode_dirs(L.ptr(dirs), n, int(bool(sphere)), float(roughness), L.ptr(X), L.stream_ptr()))
            raw = chain.forward(X, None, n, save=False)['heads'][3]
            _finish(raw, n, exp_max, gamma, out)
    return out


def rgbe_encode(img):
    """float32 CUDA tensor [..., 3] (linear radiance) -> uint8 [..., 4] Radiance RGBE on the device (nero_env_rgbe): with v the largest channel
    = m 2^e, m in [0.5, 1), the bytes are trunc(c 2^(8 - e)) and e + 128; (0, 0, 0, 0) when v < 1e-32; negative channels count as 0"""
    if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.float32 and img.dim() >= 1 and img.shape[-1] == 3):
        raise ValueError('rgbe_encode: a float32 CUDA tensor [..., 3] is expected')
    img = img.detach().contiguous()
    n = img.numel() // 3
    with torch.cuda.device(img.device):
        out = torch.empty(img.shape[:-1] + (4,), dtype=torch.uint8, device=img.device)
        L.check(_lib.nero_env_rgbe(L.ptr(img), n, L.ptr(out), L.stream_ptr()))
    return out


def rgbe_encode_host(img):
    """the same definition for a host array (numpy float32 [..., 3] -> uint8 [..., 4]): what write_hdr uses for images that are not on a GPU"""
    x = np.ascontiguousarray(img, dtype=np.float32)
    if x.ndim < 1 or x.shape[-1] != 3:
        raise ValueError(f'rgbe_encode_host: [..., 3] expected, got {x.shape}')
    ch = np.where(x > 0, x, np.float32(0)).astype(np.float32)
    v = ch.max(-1)
    _, e = np.frexp(v)
    e = np.where(np.isfinite(v), np.minimum(e, 127), 127).astype(np.int32)
    with np.errstate(invalid='ignore', over='ignore'):          # (pixels below RGBE_MIN are zeroed at the end, whatever their scale)
        scale = np.ldexp(np.float32(1), 8 - e).astype(np.float32)
        byts = np.minimum(ch * scale[..., None], np.float32(255))
    out = np.zeros(x.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.nan_to_num(byts, nan=0.0).astype(np.uint8)
    out[..., 3] = (e + 128).astype(np.uint8)
    out[v < np.float32(RGBE_MIN)] = 0
    return out


def rgbe_decode(rgbe):
    """uint8 [..., 4] (numpy or tensor) -> float32 numpy [..., 3]: byte 2^(E - 136), exact in float32"""
    b = rgbe.detach().cpu().numpy() if torch.is_tensor(rgbe) else np.asarray(rgbe)
    if b.dtype != np.uint8 or b.shape[-1] != 4:
        raise ValueError('rgbe_decode: uint8 [..., 4] expected')
    return np.ldexp(b[..., :3].astype(np.float32), b[..., 3:4].astype(np.int32) - 136).astype(np.float32)


# ---- the Radiance file ------------------------------------------------------------------------------------------------------------------------
def write_hdr(path, img):
    """img [h, w, 3] float32 (a CUDA tensor: encoded on the device; a host tensor or numpy array: rgbe_encode_host), linear radiance ->
    a Radiance picture: `#?RADIANCE`, `FORMAT=32-bit_rle_rgbe`, a blank line, `-Y h +X w`, then h flat (not run-length encoded) scanlines of
    w RGBE pixels, row 0 first.  An image with a non-finite value or a value outside [0, 2^127) raises ValueError before anything is
    written.  -> the RGBE bytes uint8 numpy [h, w, 4] that went into the file."""
    if torch.is_tensor(img):
        if img.dim() != 3 or img.shape[-1] != 3:
            raise ValueError(f'write_hdr: [h, w, 3] expected, got {tuple(img.shape)}')
        t = img.detach().to(torch.float32)
        ok = bool((torch.isfinite(t) & (t >= 0) & (t < RGBE_LIMIT)).all()) if t.numel() else True
    else:
        t = np.asarray(img)
        if t.ndim != 3 or t.shape[-1] != 3:
            raise ValueError(f'write_hdr: [h, w, 3] expected, got {t.shape}')
        with np.errstate(invalid='ignore'):
            ok = bool((np.isfinite(t) & (t >= 0) & (t < RGBE_LIMIT)).all())
        t = t.astype(np.float32)
    if not ok:
        raise ValueError('write_hdr: the image holds a non-finite value or a value outside [0, 2^127): not representable as RGBE')
    h, w = int(t.shape[0]), int(t.shape[1])
    if h < 1 or w < 1:
        raise ValueError(f'write_hdr: an empty image {h} x {w}')
    rgbe = rgbe_encode(t).cpu().numpy() if (torch.is_tensor(t) and t.is_cuda) else rgbe_encode_host(t.numpy() if torch.is_tensor(t) else t)
    with open(path, 'wb') as fh:
        fh.write(b'#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n' + f'-Y {h} +X {w}\n'.encode('ascii'))
        fh.write(np.ascontiguousarray(rgbe).tobytes())
    return rgbe


def _read_scanline_rle(data, at, w):
    """one new-style run-length scanline (2, 2, w >> 8, w & 255, then four channel planes of runs / literals) -> ([w, 4], new offset)"""
    line = np.empty((w, 4), np.uint8)
    for c in range(4):
        x = 0
        while x < w:
            if at >= len(data):
                raise ValueError('read_hdr: the file ends inside a run-length scanline')
            k = data[at]
            at += 1
            if k > 128:                                   # a run: k - 128 copies of the next byte
                k -= 128
                if k == 0 or x + k > w or at >= len(data):
                    raise ValueError('read_hdr: a run leaves its scanline')
                line[x:x + k, c] = data[at]
                at += 1
            else:                                         # k literal bytes
                if k == 0 or x + k > w or at + k > len(data):
                    raise ValueError('read_hdr: a literal block leaves its scanline')
                line[x:x + k, c] = np.frombuffer(data, np.uint8, k, at)
                at += k
            x += k
    return line, at


def read_hdr(path, return_rgbe=False):
    """a Radiance picture with `-Y h +X w` orientation, flat or new-style run-length scanlines (each scanline decides for itself)
    -> float32 numpy [h, w, 3] = byte 2^(E - 136); with return_rgbe also the bytes uint8 [h, w, 4]"""
    data = open(path, 'rb').read()
    if not data.startswith(b'#?'):
        raise ValueError(f'read_hdr: {path} is not a Radiance picture')
    end = data.find(b'\n\n')
    if end < 0:
        raise ValueError('read_hdr: no end of header')
    header = data[:end].decode('ascii', 'replace').split('\n')
    fmt = [ln.split('=', 1)[1].strip() for ln in header if ln.startswith('FORMAT=')]
    if fmt and fmt[0] != '32-bit_rle_rgbe':
        raise ValueError(f'read_hdr: FORMAT {fmt[0]!r} is not supported (32-bit_rle_rgbe only)')
    eol = data.find(b'\n', end + 2)
    res = data[end + 2:eol].decode('ascii', 'replace').split()
    if len(res) != 4 or res[0] != '-Y' or res[2] != '+X':
        raise ValueError(f'read_hdr: resolution line {" ".join(res)!r}: only "-Y h +X w" is supported')
    h, w = int(res[1]), int(res[3])
    if h < 1 or w < 1:
        raise ValueError(f'read_hdr: an empty picture {h} x {w}')
    at = eol + 1
    rgbe = np.empty((h, w, 4), np.uint8)
    for y in range(h):
        if (8 <= w < 32768 and at + 4 <= len(data) and data[at] == 2 and data[at + 1] == 2 and (data[at + 2] << 8 | data[at + 3]) == w):
            rgbe[y], at = _read_scanline_rle(data, at + 4, w)
        else:
            if at + 4 * w > len(data):
                raise ValueError('read_hdr: the file ends inside a scanline')
            rgbe[y] = np.frombuffer(data, np.uint8, 4 * w, at).reshape(w, 4)
            at += 4 * w
    img = rgbe_decode(rgbe)
    return (img, rgbe) if return_rgbe else img
