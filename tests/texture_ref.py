"""numpy restatement of the contracts of nero_amd/csrc/texture.hip (include/nero_hip.h, nero_uv_* / nero_tex_*): slow and obvious, the thing the
kernels are compared with.  Everything is exact integer arithmetic or float64."""
import numpy as np

COORD_LIMIT = float(1 << 30)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------
def snap(vt, h, w):
    """-> float64 [nvt, 2] of rint(double(u) w 256), rint(double(v) h 256) (kept as float64 so that non-finite values survive)"""
    vt = np.asarray(vt, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([np.rint(vt[:, 0] * w * 256), np.rint(vt[:, 1] * h * 256)], -1)


def triangle(snapped, face):
    """-> (x [3], y [3] python ints wound so that A > 0, A, swapped) or None when the triangle covers nothing by rule"""
    p = snapped[np.asarray(face)]
    if not np.all(np.abs(p) <= COORD_LIMIT):                        # (NaN compares false)
        return None
    x = [int(v) for v in p[:, 0]]
    y = [int(v) for v in p[:, 1]]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    if A == 0:
        return None
    swapped = A < 0
    if swapped:
        x[1], x[2], y[1], y[2], A = x[2], x[1], y[2], y[1], -A
    return x, y, A, swapped


def edge(ax, ay, bx, by, px, py):
    """edge function of a -> b at the points (px, py) (int64 arrays) and the inside decision with the ownership rule"""
    dx, dy = bx - ax, by - ay
    e = dx * (py - ay) - dy * (px - ax)
    owns = dy < 0 or (dy == 0 and dx > 0)
    return e, (e > 0) | ((e == 0) & owns)


def edges_at(tri, px, py):
    """e[k] = edge function opposite vertex k, inside mask"""
    x, y, _, _ = tri
    e0, i0 = edge(x[1], y[1], x[2], y[2], px, py)
    e1, i1 = edge(x[2], y[2], x[0], y[0], px, py)
    e2, i2 = edge(x[0], y[0], x[1], y[1], px, py)
    return (e0, e1, e2), i0 & i1 & i2


def raster(vt, ft, h, w, count=False):
    """tri_id int32 [h, w], -1 where uncovered; the lowest triangle index wins.  count: also how many triangles cover each texel"""
    ft = np.asarray(ft, dtype=np.int64).reshape(-1, 3)
    S = snap(vt, h, w)
    tri_id = np.full((h, w), -1, np.int32)
    cover = np.zeros((h, w), np.int32)
    for t, face in enumerate(ft):
        tri = triangle(S, face)
        if tri is None:
            continue
        x, y, _, _ = tri
        x_lo, x_hi = max(0, -((128 - min(x)) // 256)), min(w - 1, (max(x) - 128) // 256)          # ceil / floor of (c - 128) / 256
        y_lo, y_hi = max(0, -((128 - min(y)) // 256)), min(h - 1, (max(y) - 128) // 256)
        if x_lo > x_hi or y_lo > y_hi:
            continue
        yy, xx = np.meshgrid(np.arange(y_lo, y_hi + 1, dtype=np.int64), np.arange(x_lo, x_hi + 1, dtype=np.int64), indexing='ij')
        _, inside = edges_at(tri, 256 * xx + 128, 256 * yy + 128)
        sub = tri_id[y_lo:y_hi + 1, x_lo:x_hi + 1]
        sub[inside & (sub < 0)] = t
        cover[y_lo:y_hi + 1, x_lo:x_hi + 1] += inside
    return (tri_id, cover) if count else tri_id


def interp(tri_id, vt, ft, attr, fa):
    """-> (texel int32 [n] ascending, values float64 [n, C] = (e0 a0 + e1 a1 + e2 a2) / A, NOT yet rounded to float32, bary float64 [n, 3])"""
    h, w = tri_id.shape
    ft = np.asarray(ft, dtype=np.int64).reshape(-1, 3)
    fa = np.asarray(fa, dtype=np.int64).reshape(-1, 3)
    attr = np.asarray(attr, dtype=np.float32).astype(np.float64)
    S = snap(vt, h, w)
    texel = np.nonzero(tri_id.reshape(-1) >= 0)[0].astype(np.int32)
    vals = np.zeros((len(texel), attr.shape[1]))
    bary = np.zeros((len(texel), 3))
    for k, p in enumerate(texel):
        t = int(tri_id.reshape(-1)[p])
        tri = triangle(S, ft[t])
        (e0, e1, e2), _ = edges_at(tri, np.int64(256 * (int(p) % w) + 128), np.int64(256 * (int(p) // w) + 128))
        A, swapped = tri[2], tri[3]
        ia = fa[t][[0, 2, 1]] if swapped else fa[t]
        e = [np.float64(int(e0)), np.float64(int(e1)), np.float64(int(e2))]
        vals[k] = (e[0] * attr[ia[0]] + e[1] * attr[ia[1]] + e[2] * attr[ia[2]]) / np.float64(A)
        b = np.array(e) / np.float64(A)
        bary[k] = b[[0, 2, 1]] if swapped else b                    # weights of the face's vertices in the face's own order
    return texel, vals, bary


# ---- quantisation -----------------------------------------------------------------------------------------------------------------------------
def srgb255(x):
    """float64: linear_to_srgb (utils/raw_utils.py:11-15) of x clamped to [0, 1] (NaN -> 0), times 255"""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(x > 0, np.where(x < 1, x, 1.0), 0.0)
    eps = np.finfo(np.float32).eps
    return np.where(x <= 0.0031308, 323 / 25 * x, (211 * np.maximum(eps, x) ** (5 / 12) - 11) / 200) * 255


def quantize(values, texel, h, w):
    values = np.asarray(values)
    tex = np.zeros((h * w, values.shape[1]), np.uint8)
    tex[np.asarray(texel)] = srgb255(values).astype(np.uint8)
    return tex.reshape(h, w, -1)


# ---- regions ------------------------------------------------------------------------------------------------------------------------------------
def cityblock_to(target):
    """city-block distance of every texel to the nearest True texel of `target` (a large number when there is none): four sweeps"""
    h, w = target.shape
    big = 1 << 20
    d = np.where(target, 0, big).astype(np.int64)
    for x in range(1, w):
        d[:, x] = np.minimum(d[:, x], d[:, x - 1] + 1)
    for x in range(w - 2, -1, -1):
        d[:, x] = np.minimum(d[:, x], d[:, x + 1] + 1)
    for y in range(1, h):
        d[y] = np.minimum(d[y], d[y - 1] + 1)
    for y in range(h - 2, -1, -1):
        d[y] = np.minimum(d[y], d[y + 1] + 1)
    return d


def regions(mask, pad=32, border=3):
    """0 nothing, 1 covered interior, 2 covered within `border` of an uncovered texel (outside the image = uncovered), 3 uncovered within `pad`
    of a covered texel; distances are city-block"""
    mask = np.asarray(mask) != 0
    to_cov = cityblock_to(mask)
    to_unc = cityblock_to(~np.pad(mask, 1, constant_values=False))[1:-1, 1:-1]
    r = np.zeros(mask.shape, np.uint8)
    r[mask] = 1
    r[mask & (to_unc <= border)] = 2
    r[~mask & (to_cov <= pad)] = 3
    return r


# ---- fill -----------------------------------------------------------------------------------------------------------------------------------------
def fill(tex, region, pad=32, details=False):
    """-> (filled copy of tex [h, w, C], src int32 [h, w]: the source's row-major index or -1).  Nearest = smallest integer squared Euclidean
    distance among the region-2 texels within `pad` rows and `pad` columns, ties to the lowest row-major index.  details: also
    (d2 int64 per fill texel in row-major order, n_tied = how many search texels share that minimum)"""
    region = np.asarray(region)
    h, w = region.shape
    out = np.array(tex, copy=True).reshape(h, w, -1)
    src = np.full((h, w), -1, np.int32)
    sy, sx = np.nonzero(region == 2)
    sidx = sy.astype(np.int64) * w + sx
    fy, fx = np.nonzero(region == 3)
    d2s, ties = np.full(len(fy), -1, np.int64), np.zeros(len(fy), np.int64)
    flat_in = np.asarray(tex).reshape(h * w, -1)
    for k, (y, x) in enumerate(zip(fy, fx)):
        lo, hi = np.searchsorted(sy, y - pad), np.searchsorted(sy, y + pad, side='right')       # (sy ascends: the rows of the window)
        dy, dx = sy[lo:hi] - y, sx[lo:hi] - x
        ok = np.abs(dx) <= pad
        if not ok.any():
            continue
        d2 = (dy * dy + dx * dx)[ok]
        cand = sidx[lo:hi][ok]
        m = d2.min()
        best = cand[d2 == m].min()
        src[y, x] = best
        out[y, x] = flat_in[best]
        d2s[k], ties[k] = m, int((d2 == m).sum())
    out = out.reshape(np.asarray(tex).shape)
    return (out, src, d2s, ties) if details else (out, src)


def downsample2(tex):
    t = np.asarray(tex).astype(np.int32)
    return ((t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2] + 2) >> 2).astype(np.uint8)


# ---- shared cases -----------------------------------------------------------------------------------------------------------------------------------
def jittered_grid(h, w, nx, ny, seed):
    """a triangulation of the unit square: (nx + 1) x (ny + 1) vertices, the inner ones jittered, some snapped onto texel centres, each quad
    split along a random diagonal, every triangle with a random winding -> (vt float32, ft int32)"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing='xy')
    p = np.stack([gx, gy], -1)
    jit = (rng.random(p.shape) - 0.5) * 0.6 / np.array([nx, ny])
    p[1:-1, 1:-1] += jit[1:-1, 1:-1]
    onc = rng.random(p.shape[:2]) < 0.3                              # onto texel centres
    onc[0] = onc[-1] = False
    onc[:, 0] = onc[:, -1] = False
    onc[1, 1] = True                                                 # at least one, whatever the seed
    cen = (np.floor(p * np.array([w, h])) + 0.5) / np.array([w, h])
    p[onc] = cen[onc]
    vt = p.reshape(-1, 2).astype(np.float32)
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            tris = [(a, b, c), (a, c, d)] if rng.random() < 0.5 else [(a, b, d), (b, c, d)]
            for t in tris:
                faces.append(t if rng.random() < 0.5 else (t[0], t[2], t[1]))
    return vt, np.array(faces, np.int32)


GRID_CASES = [(8, 8, 3, 3, 1), (16, 16, 5, 4, 2), (33, 20, 7, 5, 3)]           # (h, w, nx, ny, seed)


def special_cases():
    """name -> (vt, ft, h, w, expectation); expectation: 'single' (every centre of the square covered exactly once), 'empty', or 'lowest'"""
    f32 = lambda a: np.array(a, np.float32)
    out = {}
    # a square split along the diagonal through the texel centres (i + .5, i + .5): the shared edge owns each of them exactly once
    out['diagonal_through_centres'] = (f32([[0, 0], [1, 0], [1, 1], [0, 1]]), np.array([[0, 1, 2], [0, 3, 2]], np.int32), 8, 8, 'single')
    # an axis-aligned shared edge at v = 2.5 / 8: through a whole row of centres
    out['edge_along_a_row_of_centres'] = (f32([[0, 0], [1, 0], [1, 2.5 / 8], [0, 2.5 / 8], [1, 1], [0, 1]]),
                                          np.array([[0, 1, 2], [0, 2, 3], [3, 2, 4], [3, 5, 4]], np.int32), 8, 8, 'single')
    out['degenerate'] = (f32([[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]]), np.array([[0, 1, 2]], np.int32), 16, 16, 'empty')
    # between the centres (1.5, 1.5) and (2.5, 2.5) of an 8 x 8 map
    out['sub_texel_between_centres'] = (f32([[1.6 / 8, 1.6 / 8], [2.4 / 8, 1.7 / 8], [1.9 / 8, 2.4 / 8]]), np.array([[0, 1, 2]], np.int32), 8, 8, 'empty')
    out['overlap_lowest_wins'] = (f32([[0, 0], [1, 0], [0, 1], [1, 1], [0.2, 0.1], [0.9, 0.3], [0.3, 0.95]]),
                                  np.array([[4, 5, 6], [0, 1, 2], [1, 3, 2]], np.int32), 16, 16, 'lowest')
    return out


def gutter_mask(h, w, seed):
    """the seeded test masks: six random rectangles, a 5 x 9 block in the corner, one isolated texel, 0.2 % random specks"""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), bool)
    for _ in range(6):
        rh, rw = rng.integers(4, h // 3), rng.integers(4, w // 3)
        y, x = rng.integers(0, h - rh), rng.integers(0, w - rw)
        m[y:y + rh, x:x + rw] = True
    m[:5, :9] = True
    m[h - 7, w // 2] = True
    m |= rng.random((h, w)) < 0.002
    return m


GUTTER_MASKS = [(96, 128, 11), (80, 80, 12), (150, 70, 13)]                     # (h, w, seed)
GUTTER_PADS = (32, 5)
