"""numpy / scipy restatements of the validation metrics (nero_amd/metrics.py, nero_amd/csrc/image_metrics.hip): test infrastructure, never
imported from nero_amd/.

  color_map_backward  utils/base_utils.py:453-456
  psnr_ref32          the reference's formula with its float32 means (network/metrics.py:11-17)
  psnr_exact          the same quantity from the int64 sum of squared differences, in float64
  ssim_ref            skimage.metrics.structural_similarity(gt, pr, win_size=11, channel_axis=2, data_range=255) as its documentation and
                      the paper describe it: float64 uniform_filter(size=11) per channel, sample covariance, crop 5, mean
  ssim_int            the same with integer window sums from a summed-area table (what the kernel does)
skimage is not available to this project: ssim_ref is its statement of that algorithm, and ssim_int agrees with it to 6e-16 over the cases
below."""
import numpy as np

WIN = 11
NP = WIN * WIN
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2

# h, w: the smallest shapes at which the tiled kernel can go wrong: its tile is 32 window positions (42 pixels with the halo), walked in
# segments of 8 columns and 4 rows -- 12 has the first slid window, 21 crosses a segment in both directions
SHAPES = [(11, 11), (11, 12), (12, 11), (11, 13), (21, 21), (41, 43), (42, 42), (43, 41), (75, 53), (97, 131), (140, 270)]
CHANNELS = [1, 3]
KINDS = ['noise', 'shift8', 'same', 'white_black']


def color_map_backward(x):
    x = np.asarray(x) * 255
    return np.clip(x, a_min=0, a_max=255).astype(np.uint8)


def make_pair(kind, h, w, c, seed=0):
    """-> (gt, pr) uint8 [h, w, c], seeded"""
    rg = np.random.default_rng([seed, h, w, c, KINDS.index(kind)])
    gt = rg.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == 'noise':                                     # uniform noise against uniform noise
        return gt, rg.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == 'shift8':                                    # an image against itself +- 8
        d = rg.integers(-8, 9, (h, w, c))
        return gt, np.clip(gt.astype(np.int64) + d, 0, 255).astype(np.uint8)
    if kind == 'same':
        return gt, gt.copy()
    if kind == 'white_black':
        return np.full((h, w, c), 255, np.uint8), np.zeros((h, w, c), np.uint8)
    raise ValueError(kind)


def sse_exact(gt, pr):
    d = gt.astype(np.int64) - pr.astype(np.int64)
    return int((d * d).sum())


def psnr_exact(gt, pr):
    sse = sse_exact(gt, pr)
    if sse == 0:
        return float('inf')
    return float(10.0 * np.log10(65025.0 / (np.float64(sse) / np.float64(gt.size))))


def psnr_ref32(gt, pr):
    c = gt.shape[-1]
    a = gt.reshape([-1, c]).astype(np.float32)
    b = pr.reshape([-1, c]).astype(np.float32)
    mse = np.mean((a - b) ** 2, 0)
    mse = np.mean(mse)
    with np.errstate(divide='ignore'):
        return 10 * np.log10(255 * 255 / mse)


def _ssim_from_moments(ux, uy, uxx, uyy, uxy):
    cov_norm = NP / (NP - 1.0)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_ref(gt, pr):
    """-> (mean over channels, per channel [c])"""
    from scipy.ndimage import uniform_filter
    per = []
    for ch in range(gt.shape[-1]):
        x, y = gt[..., ch].astype(np.float64), pr[..., ch].astype(np.float64)
        f = lambda a: uniform_filter(a, size=WIN)
        S = _ssim_from_moments(f(x), f(y), f(x * x), f(y * y), f(x * y))
        pad = (WIN - 1) // 2
        per.append(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64))
    per = np.asarray(per, np.float64)
    return float(per.mean()), per


def _window_sums(a):
    """a int64 [h, w] -> the sums over every 11 x 11 window inside the image, int64 [h - 10, w - 10]"""
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    return s[WIN:, WIN:] - s[:-WIN, WIN:] - s[WIN:, :-WIN] + s[:-WIN, :-WIN]


def ssim_int(gt, pr):
    """-> (mean over channels, per channel [c]); every window sum an exact integer"""
    per = []
    for ch in range(gt.shape[-1]):
        x, y = gt[..., ch].astype(np.int64), pr[..., ch].astype(np.int64)
        sx, sy, sxx, syy, sxy = (_window_sums(a) for a in (x, y, x * x, y * y, x * y))
        a1 = (2 * sx * sy) / float(NP * NP) + C1
        a2 = (2 * (NP * sxy - sx * sy)) / float(NP * (NP - 1)) + C2
        b1 = (sx * sx + sy * sy) / float(NP * NP) + C1
        b2 = (NP * sxx - sx * sx + NP * syy - sy * sy) / float(NP * (NP - 1)) + C2
        per.append(((a1 * a2) / (b1 * b2)).mean(dtype=np.float64))
    per = np.asarray(per, np.float64)
    return float(per.mean()), per


def concat_images_list(*imgs, vert=False):
    """numpy statement of utils/draw_utils.py:163-183"""
    out = imgs[0]
    for im in imgs[1:]:
        if not vert:
            h = max(out.shape[0], im.shape[0])
            out, im = (np.pad(a, ((0, h - a.shape[0]), (0, 0), (0, 0))) for a in (out, im))
            out = np.concatenate([out, im], 1)
        else:
            w = max(out.shape[1], im.shape[1])
            out, im = (np.pad(a, ((0, 0), (0, w - a.shape[1]), (0, 0))) for a in (out, im))
            out = np.concatenate([out, im], 0)
    return out
