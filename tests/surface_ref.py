"""numpy restatement of the surface sampler's contract (include/nero_hip_surface.h): integer weights and their running sum in
uint64, searchsorted(side='right') for the triangle, float64 positions rounded once to float32.  Every float64 operation is one numpy
operation, so each is rounded on its own, as the kernels' are."""
import numpy as np

M32 = 0xffffffff
STEP = 0x68E31DA4


def lowbias32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def hashes(i, seed):
    """h1..h4 of the sample indices i, uint64 arrays holding 32-bit values"""
    i = np.asarray(i, np.uint64)
    h1 = lowbias32((i * 0x9E3779B9 + (int(seed) & M32)) & M32)
    h2 = lowbias32((h1 + STEP) & M32)
    h3 = lowbias32((h2 + STEP) & M32)
    h4 = lowbias32((h3 + STEP) & M32)
    return h1, h2, h3, h4


def _corners(vertices, triangles):
    """-> (valid [T] bool, p [T,3,3] float64 with the corners of the invalid triangles set to 0)"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    valid = ((t >= 0) & (t < len(v))).all(1)
    p = v[np.where(valid[:, None], t, 0)].astype(np.float64)
    return valid, p


def cross_norm(vertices, triangles):
    """-> (valid, p, c [T,3], len [T]): c = (p1 - p0) x (p2 - p0), len = sqrt((cx cx + cy cy) + cz cz), term by term"""
    valid, p = _corners(vertices, triangles)
    u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all='ignore'):
        c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
        ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return valid, p, c, ln


def bit_length(x):
    return int(x).bit_length()


def weight_bits(T):
    return min(40, 62 - bit_length(T - 1))


def surface_cdf(vertices, triangles):
    """-> dict: w, cdf (uint64 [T]), total, zero_weight, e, B (ints), a2 (float64 [T]), area"""
    valid, _, _, ln = cross_norm(vertices, triangles)
    a2 = np.where(valid & np.isfinite(ln), ln, 0.0)
    T = len(a2)
    mx = float(a2.max())
    B = weight_bits(T)
    e = int(np.frexp(mx)[1]) if mx > 0 else 0
    w = np.floor(np.ldexp(a2, B - e)).astype(np.uint64) if mx > 0 else np.zeros(T, np.uint64)
    cdf = np.cumsum(w, dtype=np.uint64)
    total = int(cdf[-1])
    assert total < 2 ** 62
    return {'w': w, 'cdf': cdf, 'total': total, 'zero_weight': int((w == 0).sum()), 'e': e, 'B': B, 'a2': a2,
            'area': total * 2.0 ** (e - B) / 2}


def sample(vertices, triangles, cdf, total, first, n, n_total, seed=0, stratified=True):
    """samples [first, first + n) of n_total over a given running sum (the device's own, or surface_cdf's) -> dict: pts [n,3] float32, face
    [n] int32, bary [n,2] float32, normal [n,3] float32, and b [n,3] float64 (b0, b1, b2)"""
    cdf = np.asarray(cdf).astype(np.uint64)
    total = int(total)
    if total == 0:
        return {'pts': np.zeros((n, 3), np.float32), 'face': np.full(n, -1, np.int32), 'bary': np.zeros((n, 2), np.float32),
                'normal': np.zeros((n, 3), np.float32), 'b': np.zeros((n, 3))}
    i = np.arange(first, first + n, dtype=np.uint64)
    h1, h2, h3, h4 = hashes(i, seed)
    if stratified:
        u = (i.astype(np.float64) + (h1 >> 8).astype(np.float64) * 2.0 ** -24) / np.float64(n_total)
    else:
        u = ((h1 << 21) | (h4 >> 11)).astype(np.float64) * 2.0 ** -53
    target = np.minimum((u * np.float64(total)).astype(np.uint64), np.uint64(total - 1))
    face = np.searchsorted(cdf, target, side='right')
    _, p, c, ln = cross_norm(vertices, np.asarray(triangles, np.int64).reshape(-1, 3)[face])
    r1, r2 = (h2 >> 8).astype(np.float64) * 2.0 ** -24, (h3 >> 8).astype(np.float64) * 2.0 ** -24
    su = np.sqrt(r1)
    b0, b1, b2 = 1.0 - su, su * (1.0 - r2), su * r2
    pts = (b0[:, None] * p[:, 0] + b1[:, None] * p[:, 1]) + b2[:, None] * p[:, 2]
    return {'pts': pts.astype(np.float32), 'face': face.astype(np.int32), 'bary': np.stack([b1, b2], -1).astype(np.float32),
            'normal': (c / ln[:, None]).astype(np.float32), 'b': np.stack([b0, b1, b2], -1)}


def squashed_icosphere():
    """icosphere(2, 0.5) scaled by (1, 0.6, 0.25): 320 triangles whose areas span a ratio of about 4"""
    from nero_amd.synthetic import icosphere
    v, f = icosphere(2, 0.5)
    return (v * np.asarray([1.0, 0.6, 0.25], np.float32)).astype(np.float32), f


def degenerate_mesh():
    """the unit square's two triangles among: a zero-area triangle (a repeated vertex), one with collinear corners, two with an index out of
    range, one over a NaN vertex and one over an infinite one -> (vertices, triangles, the faces that may be chosen)"""
    v = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [np.inf, 1, 1]], np.float32)
    f = np.asarray([[0, 1, 1], [0, 1, 2], [0, 1, 4], [0, 1, 7], [-1, 1, 2], [0, 2, 3], [0, 1, 5], [1, 2, 6]], np.int32)
    return v, f, (1, 5)
