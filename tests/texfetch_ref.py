"""A numpy restatement of include/nero_hip_texfetch.h (nero_amd/csrc/tex_fetch.hip), generic over the dtype, with one numpy operation per
device operation and in the device's order: in float32 it is what the kernels compute bit for bit, in float64 it is what they are measured
against.  Also the inputs the CPU and the GPU tier share (fetch_case), so that the tolerance of the GPU tier is measured on the CPU over the
very inputs it is applied to."""
import numpy as np

SIZES = ((1, 1), (2, 2), (4, 2), (6, 10), (8, 8), (64, 64), (96, 80))          # (h, w) of the random maps
NS = (0, 1, 63, 64, 65, 1000)                                                    # hits per call
# (spread, lod_bias): level 0 only; a footprint of up to some tens of texels; the same one level up and one down; the top level pinned
LODS = ((0.0, 0.0), (0.25, 0.0), (0.25, 1.0), (0.25, -1.0), (1e30, 0.0), (float('inf'), 0.0))
# max |float32 restatement - float64 restatement| of mat5 over every fetch_case of SIZES x NS x LODS, measured on the CPU
# (tests/test_tex_fetch_cpu.py measures it again); the GPU is allowed GPU_FACTOR times that against the float64 restatement.  The kernel
# orders nothing differently from the float32 restatement, so the margin only covers sqrtf and division corner cases.
F32_FLOOR = 1.62e-5                                                             # measured 1.6156e-5 (absolute; the values lie in [0, 1])
GPU_FACTOR = 4.0
NO_OWNER = 2 ** 31 - 1


def srgb_lut():
    """float32 [256]: the float64 inverse of linear_to_srgb at b / 255, rounded once"""
    s = np.arange(256, dtype=np.float64) / 255.0
    return np.where(s <= 0.04045, s * 25.0 / 323.0, ((200.0 * s + 11.0) / 211.0) ** 2.4).astype(np.float32)


def linear_to_srgb(x):
    """float64: this project's curve (nero_amd.renderer.linear_to_srgb)"""
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, 323.0 / 25.0 * x, (211.0 * np.maximum(x, np.finfo(np.float32).eps) ** (5.0 / 12.0) - 11.0) / 200.0)


def levels(h, w):
    n = 1
    while n < 15 and h % 2 == 0 and w % 2 == 0:
        h, w, n = h // 2, w // 2, n + 1
    return n


def pack(albedo, metallic, roughness):
    """-> uint8 [h,w,8]: (r, g, b, metallic, roughness, 0, 0, 0)"""
    h, w = metallic.shape
    rec = np.zeros((h, w, 8), np.uint8)
    rec[..., 0:3], rec[..., 3], rec[..., 4] = albedo, metallic, roughness
    return rec


def down2(x):
    """uint8 [2h,2w,C] -> [h,w,C]: (a + b + c + d + 2) >> 2"""
    x = x.astype(np.uint16)
    return ((x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(albedo, metallic, roughness):
    """-> the list of levels, uint8 [h >> k, w >> k, 8]"""
    out = [pack(albedo, metallic, roughness)]
    for _ in range(1, levels(*metallic.shape)):
        out.append(down2(out[-1]))
    return out


def face_scale(verts, tris, vt, ft, h, w, dtype=np.float32):
    D = dtype
    tris, ft = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(ft, np.int64).reshape(-1, 3)
    V, Vt, T = len(verts), len(vt), len(tris)
    out = np.zeros(T, D)
    ok = ((tris >= 0) & (tris < V)).all(1) & ((ft >= 0) & (ft < Vt)).all(1)
    i, j = tris[ok], ft[ok]
    P, U = np.asarray(verts).astype(D), np.asarray(vt).astype(D)
    with np.errstate(all='ignore'):
        ax, ay = (U[j[:, 1], 0] - U[j[:, 0], 0]) * D(w), (U[j[:, 1], 1] - U[j[:, 0], 1]) * D(h)
        bx, by = (U[j[:, 2], 0] - U[j[:, 0], 0]) * D(w), (U[j[:, 2], 1] - U[j[:, 0], 1]) * D(h)
        a_uv = np.abs(ax * by - ay * bx)
        e, g = P[i[:, 1]] - P[i[:, 0]], P[i[:, 2]] - P[i[:, 0]]
        cx, cy, cz = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1], e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2], e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
        a_world = np.sqrt((cx * cx + cy * cy) + cz * cz)
        ratio = a_uv / a_world
        good = (a_uv != 0) & (a_world != 0) & np.isfinite(ratio)
        out[ok] = np.where(good, np.sqrt(np.where(good, ratio, D(0))), D(0))
    return out


def _axis(c, n, D):
    """a coordinate in a level n texels wide -> (i0 int64 in [-1, n], f)"""
    nf = D(n)
    with np.errstate(invalid='ignore'):
        x = np.fmin(np.fmax(c * nf - D(0.5), D(-1)), nf)                # fmax and fmin return the other operand for a NaN
    fl = np.floor(x)
    return fl.astype(np.int64), x - fl


def bilinear(level, lut, u, v, dtype=np.float32):
    """the bilinear fetch of one level at (u, v) [m] -> val [m,5] (r, g, b, metallic, alpha), x0, y0, fx, fy"""
    D = dtype
    hk, wk = level.shape[:2]
    x0, fx = _axis(u, wk, D)
    y0, fy = _axis(v, hk, D)
    xa, xb = np.clip(x0, 0, wk - 1), np.clip(x0 + 1, 0, wk - 1)
    ya, yb = np.clip(y0, 0, hk - 1), np.clip(y0 + 1, 0, hk - 1)
    dec = lambda yy, xx: lut.astype(D)[level[yy, xx, :5]]
    p00, p01, p10, p11 = dec(ya, xa), dec(ya, xb), dec(yb, xa), dec(yb, xb)
    top = p00 + fx[:, None] * (p01 - p00)
    bot = p10 + fx[:, None] * (p11 - p10)
    return top + fy[:, None] * (bot - top), x0, y0, fx, fy


def _mat5(val):
    return np.concatenate([val[:, 3:4], np.sqrt(val[:, 4:5]), val[:, 0:3]], 1)


def lod(depth, spread, scale_f, lod_scale, L, dtype=np.float32):
    """-> s, l int64, t: the level-of-detail rule"""
    D = dtype
    with np.errstate(all='ignore'):
        s = np.fmax(((np.asarray(depth).astype(D) * D(np.float32(spread))) * np.asarray(scale_f).astype(D)) * D(np.float32(lod_scale)), D(1))
        _, e = np.frexp(s)
        e = np.where(np.isinf(s), 1 << 20, e.astype(np.int64) - 1)
        l = np.minimum(e, L - 1)
        t = np.where(l < L - 1, s * np.ldexp(D(1), -l).astype(D) - D(1), D(0))
    return s, l, t.astype(D)


def fetch(levels_, lut, vt, ft, scale, face, bary, depth, spread, lod_scale, dtype=np.float32):
    """nero_tex_materials -> mat5 [n,5], dbg [n,8]"""
    D = dtype
    L = len(levels_)
    face = np.asarray(face, np.int64).reshape(-1)
    ft = np.asarray(ft, np.int64).reshape(-1, 3)
    n, T, Vt = len(face), len(ft), len(vt)
    mat5, dbg = np.zeros((n, 5), D), np.zeros((n, 8), D)
    okf = (face >= 0) & (face < T)
    j = ft[np.where(okf, face, 0)] if T else np.full((n, 3), -1)
    idx = np.nonzero(okf & ((j >= 0) & (j < Vt)).all(1))[0]
    if idx.size == 0:
        return mat5, dbg
    j, f = j[idx], face[idx]
    U = np.asarray(vt).astype(D)
    bu, bv = np.asarray(bary)[idx, 0].astype(D), np.asarray(bary)[idx, 1].astype(D)
    with np.errstate(invalid='ignore'):
        w0 = (D(1) - bu) - bv
        u = (w0 * U[j[:, 0], 0] + bu * U[j[:, 1], 0]) + bv * U[j[:, 2], 0]
        v = (w0 * U[j[:, 0], 1] + bu * U[j[:, 1], 1]) + bv * U[j[:, 2], 1]
    _, l, t = lod(np.asarray(depth)[idx], spread, np.asarray(scale)[f], lod_scale, L, D)
    val = np.zeros((len(idx), 5), D)
    d = np.zeros((len(idx), 8), D)
    for k in np.unique(l):
        at = np.nonzero(l == k)[0]
        val[at], x0, y0, fx, fy = bilinear(levels_[k], lut, u[at], v[at], D)
        d[at] = np.stack([l[at].astype(D), t[at], x0.astype(D), y0.astype(D), fx, fy, u[at], v[at]], 1)
        up = at[t[at] != 0]
        if up.size:                                                      # (t != 0 only below the top level)
            hi = bilinear(levels_[k + 1], lut, u[up], v[up], D)[0]
            val[up] = val[up] + t[up, None] * (hi - val[up])
    mat5[idx], dbg[idx] = _mat5(val), d
    return mat5, dbg


def vertex_materials(levels_, lut, vt, tris, ft, V, dtype=np.float32):
    """nero_tex_vertex_materials -> mat5_v [V,5], owner int64 [V]"""
    D = dtype
    corner_v, corner_j = np.asarray(tris, np.int64).reshape(-1), np.asarray(ft, np.int64).reshape(-1)
    owner = np.full(V, NO_OWNER, np.int64)
    ok = (corner_v >= 0) & (corner_v < V)
    np.minimum.at(owner, corner_v[ok], np.arange(len(corner_v))[ok])
    out = np.zeros((V, 5), D)
    has = owner != NO_OWNER
    j = np.where(has, corner_j[np.where(has, owner, 0)] if len(corner_j) else -1, -1)
    at = np.nonzero((j >= 0) & (j < len(vt)))[0]
    if at.size:
        U = np.asarray(vt).astype(D)
        out[at] = _mat5(bilinear(levels_[0], lut, U[j[at], 0], U[j[at], 1], D)[0])
    return out, owner


# ---- the inputs both tiers share --------------------------------------------------------------------------------------------------------------
def random_maps(h, w, seed=0):
    g = np.random.default_rng(7000 + 131 * h + w + seed)
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h, w), dtype=np.uint8)


SPECIAL_UV = ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (-0.3, 0.4), (0.5, 1.7), (np.nan, 0.5), (0.25, np.nan), (np.inf, -np.inf), (1e30, -1e30))
VT, T_FACES = 40, 30


def fetch_case(h, w, n, seed=0):
    """the inputs of one fetch on an h x w map: a UV mesh of VT vertices and T_FACES faces -- the first UV vertices are SPECIAL_UV (exactly
    0 and 1, outside [0, 1], not finite), face k < len(SPECIAL_UV) has vertex k as its first corner, the last two faces name a UV vertex
    out of range (VT and -1) -- and n hits: the first lanes sit on first corners (barycentrics exactly (0, 0)), then a miss (face -1), a
    face == T, the two bad faces, an infinite depth and footprints of exactly 2 and 4 texels; the rest are random.  float32 / int32 arrays"""
    g = np.random.default_rng(9000 + 977 * h + 31 * w + n + seed)
    vt = g.uniform(0.0, 1.0, (VT, 2)).astype(np.float32)
    vt[:len(SPECIAL_UV)] = np.asarray(SPECIAL_UV, np.float32)
    ft = g.integers(len(SPECIAL_UV), VT, (T_FACES, 3)).astype(np.int32)
    ft[:len(SPECIAL_UV), 0] = np.arange(len(SPECIAL_UV))
    ft[-2, 1], ft[-1, 2] = VT, -1
    scale = g.uniform(0.5, 40.0, T_FACES).astype(np.float32)
    scale[len(SPECIAL_UV)], scale[len(SPECIAL_UV) + 1] = 0.0, 8.0
    face = g.integers(len(SPECIAL_UV), T_FACES - 2, n).astype(np.int32)
    bary = g.uniform(0.0, 1.0, (n, 2)).astype(np.float32)
    bary[:, 1] *= (1.0 - bary[:, 0])
    depth = g.uniform(0.5, 4.0, n).astype(np.float32)
    k = len(SPECIAL_UV)
    fixed = [(i, (0.0, 0.0), 1.0) for i in range(k)] + [(-1, (0.3, 0.3), 1.0), (T_FACES, (0.3, 0.3), 1.0), (T_FACES - 2, (0.2, 0.5), 1.0),
                                                         (T_FACES - 1, (0.2, 0.5), 1.0), (k + 2, (0.25, 0.25), np.inf), (k + 1, (0.5, 0.25), 1.0),
                                                         (k + 1, (0.25, 0.5), 2.0), (k + 2, (1.0, 0.0), 1.5), (k + 3, (0.0, 1.0), 0.75)]
    order = g.permutation(len(fixed)) if n < len(fixed) else np.arange(len(fixed))      # (a short call takes some of them)
    for lane, q in enumerate(order[:n]):
        face[lane], bary[lane], depth[lane] = fixed[q][0], fixed[q][1], fixed[q][2]
    return dict(vt=vt, ft=ft, scale=scale, face=face, bary=bary, depth=depth)


def fetch_cases():
    """every (h, w, n, spread, lod_bias) of the GPU tier's fetch test"""
    return [(h, w, n, spread, bias) for h, w in SIZES for n in NS for spread, bias in LODS]


def measure_floor():
    """max |float32 restatement - float64 restatement| of mat5 over fetch_cases(): what F32_FLOOR records"""
    lut, worst = srgb_lut(), 0.0
    for h, w in SIZES:
        lv = pyramid(*random_maps(h, w))
        for n in NS:
            c = fetch_case(h, w, n)
            for spread, bias in LODS:
                a = fetch(lv, lut, spread=spread, lod_scale=2.0 ** bias, dtype=np.float32, **c)[0]
                b = fetch(lv, lut, spread=spread, lod_scale=2.0 ** bias, dtype=np.float64, **c)[0]
                if n:
                    worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
    return worst
