"""numpy restatement of the denoiser (include/nero_hip_denoise.h), generic over the dtype: every operation below is one operation of the
kernels of nero_amd/csrc/denoise.hip, in their order, so that in float32 it performs the kernels' arithmetic (up to expf's last place) and
in float64 it is the reference they are held to.  The constants are the float32 values the kernels hold, widened; the sigmas are rounded to
float32 first, as the C ABI does.  Divisions are guarded: a sum of weights that underflows to zero copies the pixel through, never 0 / 0.

Also the analytic test scene (a sphere over a plane) of the CPU tier and a torch-free packer of the two records."""
import numpy as np

LUM = (0.2126, 0.7152, 0.0722)
C5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
C3 = (0.25, 0.5, 0.25)
EPS_DEN = 1e-6


def pack_guides(pos, normal, valid, extra=None):
    """[n,3], [n,3], [n] bool, [n,4] or None -> guide [n,8] or [n,12] float32"""
    n = len(pos)
    v = np.asarray(valid).reshape(n).astype(bool)
    cols = [np.asarray(normal, np.float32).reshape(n, 3), v.astype(np.float32)[:, None], np.asarray(pos, np.float32).reshape(n, 3),
            np.zeros((n, 1), np.float32)]
    if extra is not None:
        cols.append(np.asarray(extra, np.float32).reshape(n, 4))
    g = np.concatenate(cols, 1)
    g[~v] = 0.0
    return np.ascontiguousarray(g)


def pack_signal(rgb, var=None):
    n = len(rgb)
    return np.ascontiguousarray(np.concatenate([np.asarray(rgb, np.float32).reshape(n, 3),
                                                np.zeros((n, 1), np.float32) if var is None else np.asarray(var, np.float32).reshape(n, 1)], 1))


def _c(x, dt):
    return dt(np.float32(x))


def _lum(s, dt):
    return (_c(LUM[0], dt) * s[..., 0] + _c(LUM[1], dt) * s[..., 1]) + _c(LUM[2], dt) * s[..., 2]


class _Image:
    """the two records as [h,w,C] arrays of dtype dt, and the gather of a tap"""

    def __init__(self, guide, signal, h, w, dt):
        G = guide.shape[1] - 8
        assert G in (0, 4) and guide.shape[0] == h * w and signal.shape == (h * w, 4)
        self.h, self.w, self.G, self.dt = h, w, G, dt
        self.g = np.asarray(guide, np.float32).astype(dt).reshape(h, w, 8 + G)
        self.s = np.asarray(signal, np.float32).astype(dt).reshape(h, w, 4)
        self.valid = self.g[..., 3] != 0
        self.ys, self.xs = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing='ij')

    def tap(self, oy, ox):
        """-> (inside & valid_q [h,w], guide_q, signal_q): the pixel at (y + oy, x + ox) of every pixel; values outside are the clipped
        pixel's and masked"""
        qy, qx = self.ys + int(oy), self.xs + int(ox)
        inside = (qy >= 0) & (qy < self.h) & (qx >= 0) & (qx < self.w)
        cy, cx = np.clip(qy, 0, self.h - 1), np.clip(qx, 0, self.w - 1)
        return inside & self.valid[cy, cx], self.g[cy, cx], self.s[cy, cx]

    def guide_weight(self, gq, k, sigma_p, sigma_g):
        dt, a = self.dt, self.g
        wn = np.maximum((a[..., 0] * gq[..., 0] + a[..., 1] * gq[..., 1]) + a[..., 2] * gq[..., 2], dt(0))
        for _ in range(int(k)):
            wn = wn * wn
        dx, dy, dz = gq[..., 4] - a[..., 4], gq[..., 5] - a[..., 5], gq[..., 6] - a[..., 6]
        plane = (a[..., 0] * dx + a[..., 1] * dy) + a[..., 2] * dz
        wt = wn * np.exp(-(np.abs(plane) / _c(sigma_p, dt)))
        if self.G == 4:
            e = [a[..., 8 + c] - gq[..., 8 + c] for c in range(4)]
            d2 = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]
            sg = _c(sigma_g, dt)
            wt = wt * np.exp(-(d2 / (sg * sg)))
        return wt


def estimate_variance(guide, signal, h, w, k=6, sigma_p=0.05, sigma_g=0.1, dtype=np.float64):
    """nero_denoise_variance -> signal' [n,4] of dtype"""
    dt = np.dtype(dtype).type
    im = _Image(guide, signal, h, w, dt)
    z = lambda: np.zeros((h, w), dt)
    with np.errstate(all='ignore'):
        lum_p = _lum(im.s, dt)
        s0, s1, s2 = z(), z(), z()
        for oy in range(-3, 4):
            for ox in range(-3, 4):
                m, gq, sq = im.tap(oy, ox)
                m = m & im.valid
                wt = np.where(m, im.guide_weight(gq, k, sigma_p, sigma_g), dt(0))
                d = np.where(m, _lum(sq, dt) - lum_p, dt(0))
                s0 = s0 + wt
                s1 = s1 + wt * d
                s2 = s2 + wt * (d * d)
        ok = im.valid & (s0 > 0)
        safe = np.where(ok, s0, dt(1))
        m1, m2 = s1 / safe, s2 / safe
        var = np.maximum(m2 - m1 * m1, dt(0))
    out = im.s.copy()
    out[..., 3] = np.where(ok, var, im.s[..., 3])
    return out.reshape(h * w, 4)


def atrous_pass(guide, signal, h, w, step, k=6, sigma_l=4.0, sigma_p=0.05, sigma_g=0.1, dtype=np.float64):
    """nero_denoise_atrous -> signal' [n,4] of dtype"""
    dt = np.dtype(dtype).type
    im = _Image(guide, signal, h, w, dt)
    z = lambda: np.zeros((h, w), dt)
    with np.errstate(all='ignore'):
        va, vb = z(), z()
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                m, _, sq = im.tap(oy, ox)
                c = _c(C3[oy + 1], dt) * _c(C3[ox + 1], dt)
                va = va + np.where(m, c * sq[..., 3], dt(0))
                vb = vb + np.where(m, c, dt(0))
        gvar = va / np.where(im.valid, vb, dt(1))
        den = _c(sigma_l, dt) * np.sqrt(np.where(im.valid, gvar, dt(0))) + _c(EPS_DEN, dt)
        lum_p = _lum(im.s, dt)
        sw, sr, sg, sb, sv = z(), z(), z(), z(), z()
        for ty in range(5):
            for tx in range(5):
                m, gq, sq = im.tap((ty - 2) * int(step), (tx - 2) * int(step))
                m = m & im.valid
                gw = im.guide_weight(gq, k, sigma_p, sigma_g)
                wl = np.exp(-(np.abs(lum_p - _lum(sq, dt)) / den))
                wt = np.where(m, ((_c(C5[ty], dt) * _c(C5[tx], dt)) * gw) * wl, dt(0))
                sq = np.where(m[..., None], sq, dt(0))
                sw = sw + wt
                sr = sr + wt * sq[..., 0]
                sg = sg + wt * sq[..., 1]
                sb = sb + wt * sq[..., 2]
                sv = sv + (wt * wt) * sq[..., 3]
        ok = im.valid & (sw > 0)
        safe = np.where(ok, sw, dt(1))
        sw2 = sw * sw
        ok2 = ok & (sw2 > 0)
        out = im.s.copy()
        out[..., 0] = np.where(ok, sr / safe, im.s[..., 0])
        out[..., 1] = np.where(ok, sg / safe, im.s[..., 1])
        out[..., 2] = np.where(ok, sb / safe, im.s[..., 2])
        out[..., 3] = np.where(ok2, sv / np.where(ok2, sw2, dt(1)), im.s[..., 3])
    return out.reshape(h * w, 4)


def denoise(rgb, pos, normal, valid, h, w, extra=None, iterations=5, sigma_l=4.0, normal_pow2=6, sigma_p=0.05, sigma_g=0.1, dtype=np.float64):
    """nero_amd.denoise.denoise -> (rgb' [n,3], var [n]) of dtype"""
    guide = pack_guides(pos, normal, valid, extra)
    sig = estimate_variance(guide, pack_signal(rgb), h, w, normal_pow2, sigma_p, sigma_g, dtype)
    for it in range(int(iterations)):
        sig = atrous_pass(guide, sig, h, w, 1 << it, normal_pow2, sigma_l, sigma_p, sigma_g, dtype)
    return sig[:, :3], sig[:, 3]


def parity(got, ref32, ref64):
    """the project's convention: the distance of `got` from the float64 restatement and that of the float32 restatement from it (the floor),
    both relative to max(|value|, mean |value|) per component -> (error, floor)"""
    ref64 = np.asarray(ref64, np.float64)
    scale = np.maximum(np.abs(ref64), max(float(np.abs(ref64).mean()), np.finfo(np.float32).tiny))
    return float((np.abs(np.asarray(got, np.float64) - ref64) / scale).max()), float((np.abs(np.asarray(ref32, np.float64) - ref64) / scale).max())


# ---- the analytic scene ---------------------------------------------------------------------------------------------------------------------
def sphere_over_plane(h, w, noise=0.5, seed=1, frame=2, holes=0.0):
    """an orthographic view down -z of a sphere of radius 0.6 at (0, 0, 0.6) over the plane z = 0, the picture spanning [-1, 1]^2, the outer
    frame of `frame` pixels uncovered and a share `holes` of the others too (seeded) -> dict: pos, normal [n,3], valid [n], clean, noisy [n,3] (float32; noisy = clean (1 + noise u), u uniform
    in [-1, 1)), extra [n,4].  The clean signal is a smooth shading of each surface in a colour of its own."""
    ys, xs = np.meshgrid((np.arange(h) + 0.5) / h * 2 - 1, (np.arange(w) + 0.5) / w * 2 - 1, indexing='ij')
    r2 = xs * xs + ys * ys
    on = r2 < 0.36
    zs = np.where(on, 0.6 + np.sqrt(np.maximum(0.36 - r2, 0.0)), 0.0)
    pos = np.stack([xs, ys, zs], -1)
    nrm = np.where(on[..., None], (pos - np.asarray([0.0, 0.0, 0.6])) / 0.6, np.asarray([0.0, 0.0, 1.0]))
    light = np.asarray([0.3, 0.5, 0.81])
    light = light / np.linalg.norm(light)
    shade = 0.2 + 0.8 * np.maximum((nrm * light).sum(-1), 0.0)
    shade = np.where(on, shade, shade * (0.7 + 0.3 * xs))
    colour = np.where(on[..., None], np.asarray([0.9, 0.4, 0.2]), np.asarray([0.3, 0.6, 0.8]))
    clean = shade[..., None] * colour
    valid = np.ones((h, w), bool)
    if frame > 0:
        valid[:frame], valid[-frame:], valid[:, :frame], valid[:, -frame:] = False, False, False, False
    rng = np.random.default_rng(seed)
    if holes > 0:
        valid &= np.random.default_rng(seed + 100).uniform(size=(h, w)) >= holes
    noisy = clean * (1.0 + noise * rng.uniform(-1.0, 1.0, clean.shape))
    extra = np.stack([np.where(on, 0.3, 0.8), np.where(on, 1.0, 0.0), 0.5 + 0.1 * xs, np.zeros_like(xs)], -1)
    f = lambda a, c: np.ascontiguousarray(a.reshape(h * w, c), np.float32)
    return {'pos': f(pos, 3), 'normal': f(nrm, 3), 'valid': valid.reshape(-1), 'clean': f(clean, 3), 'noisy': f(noisy, 3), 'extra': f(extra, 4)}


def rmse(a, b, mask=None):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    return float(np.sqrt(d[mask].mean() if mask is not None else d.mean()))
