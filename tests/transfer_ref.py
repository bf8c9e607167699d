"""A numpy restatement of include/nero_transfer.h (nero_amd/csrc/detail_transfer.hip), generic over the dtype, with one numpy operation per
device operation and in the device's order: in float32 it is what the kernels compute bit for bit, in float64 it is what they are measured
against.  The level-of-detail rule and the taps are those of tests/texfetch_ref.py, as the kernels share tex_lod.h."""
import numpy as np

from tests import texfetch_ref as TR

FLAT = (128, 128, 255)
TANGENT, OBJECT = 0, 1


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- nero_mesh_attr_at ------------------------------------------------------------------------------------------------------------------------
def attr_at(attr, tris, face, bary, fill=0.0, dtype=np.float32):
    D = dtype
    attr = np.asarray(attr).astype(D)
    attr = attr.reshape(len(attr), -1)
    tris, face = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(face, np.int64).reshape(-1)
    V, T, n = len(attr), len(tris), len(face)
    out = np.full((n, attr.shape[1]), D(fill), D)
    okf = (face >= 0) & (face < T)
    idx = tris[np.where(okf, face, 0)] if T else np.full((n, 3), -1)
    at = np.nonzero(okf & ((idx >= 0) & (idx < V)).all(1))[0]
    if at.size:
        i = idx[at]
        b1, b2 = np.asarray(bary)[at, 0:1].astype(D), np.asarray(bary)[at, 1:2].astype(D)
        a0, a1, a2 = attr[i[:, 0]], attr[i[:, 1]], attr[i[:, 2]]
        with np.errstate(all='ignore'):
            out[at] = a0 + (b1 * (a1 - a0) + b2 * (a2 - a0))
    return out


# ---- nero_uv_tangents -------------------------------------------------------------------------------------------------------------------------
def bit_length(x):
    return int(x).bit_length() if x > 0 else 0


def term_bits(T):
    return min(40, 61 - bit_length(T - 1))


def face_tangents(verts, tris, vt, ft):
    """per face in float64 -> state [T] (0 contributes, 1 refused, 2 degenerate), w [T,3] = (t / |t|) |c|, weight [T] = |c|, sign [T]"""
    P, U = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(vt, np.float32).astype(np.float64).reshape(-1, 2)
    tris, ft = np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(ft, np.int64).reshape(-1, 3)
    T = len(tris)
    state = np.zeros(T, np.int64)
    w, weight, sign = np.zeros((T, 3)), np.zeros(T), np.zeros(T, np.int8)
    inr = ((tris >= 0) & (tris < len(P))).all(1) & ((ft >= 0) & (ft < len(U))).all(1)
    state[~inr] = 1
    at = np.nonzero(inr)[0]
    if at.size == 0:
        return state, w, weight, sign
    i, j = tris[at], ft[at]
    with np.errstate(all='ignore'):
        e1, e2 = P[i[:, 1]] - P[i[:, 0]], P[i[:, 2]] - P[i[:, 0]]
        du1, dv1 = U[j[:, 1], 0] - U[j[:, 0], 0], U[j[:, 1], 1] - U[j[:, 0], 1]
        du2, dv2 = U[j[:, 2], 0] - U[j[:, 0], 0], U[j[:, 2], 1] - U[j[:, 0], 1]
        det = du1 * dv2 - du2 * dv1
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        sg = np.where(det > 0, 1.0, -1.0)
        t = (e1 * dv2[:, None] - e2 * dv1[:, None]) * sg[:, None]
        refused = ~(np.isfinite(c).all(1) & np.isfinite(t).all(1))
        tl = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        cl = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        degenerate = ~refused & (~(det != 0) | np.isnan(det) | (tl == 0) | (cl == 0) | ~np.isfinite(tl) | ~np.isfinite(cl))
        ok = ~refused & ~degenerate
        state[at] = np.where(refused, 1, np.where(degenerate, 2, 0))
        w[at[ok]] = (t[ok] / tl[ok, None]) * cl[ok, None]
        weight[at[ok]] = cl[ok]
        sign[at[ok]] = np.where(det[ok] > 0, -1, 1)
    return state, w, weight, sign


def uv_tangents(verts, tris, vt, ft):
    """-> tangent float32 [Vt,3], face_sign int8 [T], info int64 [4]"""
    ft_ = np.asarray(ft, np.int64).reshape(-1, 3)
    Vt, T = len(np.asarray(vt).reshape(-1, 2)), len(ft_)
    state, w, weight, sign = face_tangents(verts, tris, vt, ft)
    ok = state == 0
    sums = np.zeros((Vt, 3), np.int64)
    e = 0
    if ok.any():
        e = int(np.frexp(weight[ok].max())[1])
        q = np.rint(np.ldexp(w[ok], term_bits(T) - e)).astype(np.int64)
        for c in range(3):
            np.add.at(sums, ft_[ok, c], q)
    zero = ~sums.any(1)
    d = sums.astype(np.float64)
    with np.errstate(all='ignore'):
        l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        tangent = np.where(zero[:, None], 0.0, d / l[:, None]).astype(np.float32)
    return tangent, sign, np.asarray([(state == 1).sum(), (state == 2).sum(), zero.sum(), e], np.int64)


# ---- THE FRAME and THE BYTES --------------------------------------------------------------------------------------------------------------------
def frame(N, T, sign, dtype=np.float32):
    """-> n, T', B [m,3], |N| [m], ok [m]"""
    D = dtype
    N, T = np.asarray(N).astype(D).reshape(-1, 3), np.asarray(T).astype(D).reshape(-1, 3)
    with np.errstate(all='ignore'):
        ln = np.sqrt(dot3(N, N))
        ok = np.isfinite(ln) & (ln != 0)
        n = N / ln[:, None]
        project = lambda X: X - dot3(X, n)[:, None] * n
        p = project(T)
        pp = dot3(p, p)
        lost = ~(pp > D(np.float32(1e-12)) * dot3(T, T))
        a = np.abs(n)
        k = np.where((a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2]), 0, np.where(a[:, 1] <= a[:, 2], 1, 2))
        p2 = project(np.eye(3, dtype=D)[k])
        p = np.where(lost[:, None], p2, p)
        pp = np.where(lost, dot3(p2, p2), pp)
        t = p / np.sqrt(pp)[:, None]
        s = np.where(np.asarray(sign).reshape(-1) < 0, D(-1), D(1))
        b = np.stack([s * (n[:, 1] * t[:, 2] - n[:, 2] * t[:, 1]), s * (n[:, 2] * t[:, 0] - n[:, 0] * t[:, 2]),
                      s * (n[:, 0] * t[:, 1] - n[:, 1] * t[:, 0])], 1)
    return n, t, b, ln, ok


def unit3(x):
    with np.errstate(all='ignore'):
        l = np.sqrt(dot3(x, x))
        return x / l[:, None], np.isfinite(l) & (l != 0)


def to_bytes(x):
    """clamp(lrintf(127 x) + 128, 1, 255)"""
    D = x.dtype.type
    with np.errstate(all='ignore'):
        r = np.rint(D(127) * x) + D(128)
        return np.fmin(np.fmax(r, D(1)), D(255)).astype(np.uint8)


def decode(b, dtype=np.float32):
    D = dtype
    return (np.asarray(b).astype(D) - D(128)) / D(127)


def encode(nrm, tan, sign, ns, valid, space, dtype=np.float32):
    """nero_nmap_encode -> bytes uint8 [n,3], invalid bool [n]"""
    D = dtype
    S = np.asarray(ns).astype(D).reshape(-1, 3)
    m = len(S)
    ok = (np.asarray(valid).reshape(-1) != 0) & np.isfinite(S).all(1)
    x = np.zeros((m, 3), D)
    x[:, 2] = 1
    with np.errstate(all='ignore'):
        if space == TANGENT:
            n, t, b, _, fok = frame(nrm, tan, sign, D)
            u, uok = unit3(np.stack([dot3(S, t), dot3(S, b), dot3(S, n)], 1))
            ok = uok & ok & fok & np.isfinite(u).all(1)
            x[ok] = u[ok]
        else:
            u, uok = unit3(S)
            ok = uok & ok & np.isfinite(u).all(1)
            mN, mok = unit3(np.asarray(nrm).astype(D).reshape(-1, 3))
            mok &= np.isfinite(mN).all(1)
            x[~ok & mok] = mN[~ok & mok]
            x[ok] = u[ok]
    return to_bytes(x), ~ok


# ---- records and pyramid ------------------------------------------------------------------------------------------------------------------------
def pyramid(nmap):
    """uint8 [h,w,3] -> the list of levels, uint8 [h >> k, w >> k, 4]"""
    h, w = nmap.shape[:2]
    rec = np.zeros((h, w, 4), np.uint8)
    rec[..., :3] = nmap
    out = [rec]
    for _ in range(1, TR.levels(h, w)):
        out.append(TR.down2(out[-1]))
    return out


def _bilinear(level, u, v, D):
    hk, wk = level.shape[:2]
    x0, fx = TR._axis(u, wk, D)
    y0, fy = TR._axis(v, hk, D)
    xa, xb = np.clip(x0, 0, wk - 1), np.clip(x0 + 1, 0, wk - 1)
    ya, yb = np.clip(y0, 0, hk - 1), np.clip(y0 + 1, 0, hk - 1)
    dec = lambda yy, xx: decode(level[yy, xx, :3], D)
    p00, p01, p10, p11 = dec(ya, xa), dec(ya, xb), dec(yb, xa), dec(yb, xb)
    top = p00 + fx[:, None] * (p01 - p00)
    bot = p10 + fx[:, None] * (p11 - p10)
    return top + fy[:, None] * (bot - top), x0, y0, fx, fy


def apply(levels_, vt, ft, scale, tangent, face_sign, face, bary, depth, nrm_in, spread, lod_scale, space=TANGENT, dtype=np.float32):
    """nero_nmap_apply -> nrm_out [n,3], dbg [n,8]"""
    D = dtype
    L = len(levels_)
    face = np.asarray(face, np.int64).reshape(-1)
    ft = np.asarray(ft, np.int64).reshape(-1, 3)
    Nin = np.asarray(nrm_in).astype(D).reshape(-1, 3)
    n, T, Vt = len(face), len(ft), len(vt)
    out, dbg = Nin.copy(), np.zeros((n, 8), D)
    okf = (face >= 0) & (face < T)
    j = ft[np.where(okf, face, 0)] if T else np.full((n, 3), -1)
    idx = np.nonzero(okf & ((j >= 0) & (j < Vt)).all(1))[0]
    if idx.size == 0:
        return out, dbg
    j, f = j[idx], face[idx]
    U, Tg = np.asarray(vt).astype(D), np.asarray(tangent).astype(D).reshape(-1, 3)
    bu, bv = np.asarray(bary)[idx, 0].astype(D), np.asarray(bary)[idx, 1].astype(D)
    with np.errstate(all='ignore'):
        w0 = (D(1) - bu) - bv
        mix = lambda X: (w0[:, None] * X[j[:, 0]] + bu[:, None] * X[j[:, 1]]) + bv[:, None] * X[j[:, 2]]
        uv = mix(U)
        u, v = uv[:, 0], uv[:, 1]
        _, l, t = TR.lod(np.asarray(depth)[idx], spread, np.asarray(scale)[f], lod_scale, L, D)
        val = np.zeros((len(idx), 3), D)
        d = np.zeros((len(idx), 8), D)
        for k in np.unique(l):
            at = np.nonzero(l == k)[0]
            val[at], x0, y0, fx, fy = _bilinear(levels_[k], u[at], v[at], D)
            d[at] = np.stack([l[at].astype(D), t[at], x0.astype(D), y0.astype(D), fx, fy, u[at], v[at]], 1)
            up = at[t[at] != 0]
            if up.size:
                hi = _bilinear(levels_[k + 1], u[up], v[up], D)[0]
                val[up] = val[up] + t[up, None] * (hi - val[up])
        N = Nin[idx]
        ok = np.ones(len(idx), bool)
        r = val
        if space == TANGENT:
            nn, tt, bb, ln, ok = frame(N, mix(Tg), np.asarray(face_sign).reshape(-1)[f], D)
            zn = val[:, 2:3] * N
            still = (val[:, 0:1] == 0) & (val[:, 1:2] == 0)                             # no tilt: z N alone, bit for bit
            r = np.where(still, zn, ((val[:, 0:1] * tt + val[:, 1:2] * bb) * ln[:, None]) + zn)
        ok = ok & np.isfinite(r).all(1) & r.any(1) & (dot3(r, N) > 0)
    out[idx] = np.where(ok[:, None], r, N)
    dbg[idx] = d
    return out, dbg


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------------
def unit_square(mirror=False):
    """two triangles over x, y in [0, 1], normal +z, with u = x (or -x + 1 when mirrored: u runs along -x) and FILE v = y, that is the
    internal row coordinate v = 1 - y -> verts, tris, vt, ft"""
    verts = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    tris = np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
    u = 1.0 - verts[:, 0] if mirror else verts[:, 0]
    vt = np.stack([u, 1.0 - verts[:, 1]], 1).astype(np.float32)
    return verts, tris, vt, tris.copy()


def angle(a, b):
    """the angle between the rows of a and b in float64, radians"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))
