"""numpy restatement of the vertex-normal contract (include/nero_hip_normals.h): fixed-point terms summed with np.add.at on
int64, np.rint (half to even), np.ldexp and np.frexp.  Every float64 operation is one numpy operation, so each is rounded on its own, as the
kernels' are; np.arctan2 is the one operation whose last places the device need not share."""
import numpy as np

AREA, ANGLE = 0, 1
WEIGHTS = {'area': AREA, 'angle': ANGLE}


def term_bits(T, weight):
    L = int(T - 1).bit_length()
    return min(40, (59 if weight == ANGLE else 61) - L)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def _norm(c):
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def faces(vertices, triangles):
    """-> (t [T,3] int64, p [T,3,3] float64 with the corners of faces out of range set to 0, c [T,3], refused [T], degenerate [T])"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    in_range = ((t >= 0) & (t < len(v))).all(1)
    p = v[np.where(in_range[:, None], t, 0)].astype(np.float64)
    with np.errstate(all='ignore'):
        c = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    refused = ~in_range | ~np.isfinite(c).all(1)
    degenerate = ~refused & (c == 0).all(1)
    return t, p, c, refused, degenerate


def vertex_sums(vertices, triangles, weight):
    """-> (sums [V,3] int64, info [refused, degenerate, ., e])"""
    weight = WEIGHTS.get(weight, weight)
    assert weight in (AREA, ANGLE)
    V = len(np.asarray(vertices).reshape(-1, 3))
    t, p, c, refused, degenerate = faces(vertices, triangles)
    ok = ~refused & ~degenerate
    B = term_bits(len(t), weight)
    sums = np.zeros((V, 3), np.int64)
    e = 0
    t, p, c = t[ok], p[ok], c[ok]
    if weight == AREA:
        if len(c):
            e = int(np.frexp(np.abs(c).max())[1])
        q = np.rint(np.ldexp(c, B - e)).astype(np.int64)
        for i in range(3):
            np.add.at(sums, t[:, i], q)
    else:
        n = c / _norm(c)[:, None]
        for i in range(3):
            a, b = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
            theta = np.arctan2(_norm(_cross(a, b)), (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
            np.add.at(sums, t[:, i], np.rint(np.ldexp(theta[:, None] * n, B)).astype(np.int64))
    assert np.abs(sums).max(initial=0) <= 2 ** 61
    return sums, [int(refused.sum()), int(degenerate.sum()), 0, e]


def finish(sums):
    """-> (normals [V,3] float32, the number of vertices written as zero)"""
    zero = (sums == 0).all(1)
    d = sums.astype(np.float64)
    with np.errstate(all='ignore'):
        out = (d / _norm(d)[:, None]).astype(np.float32)
    out[zero] = 0.0
    return out, int(zero.sum())


def vertex_normals(vertices, triangles, weight='angle'):
    """-> (normals [V,3] float32, info [4] int64 = refused faces, degenerate faces, zero vertices, e)"""
    sums, info = vertex_sums(vertices, triangles, weight)
    out, info[2] = finish(sums)
    return out, np.asarray(info, np.int64)


def face_normals(vertices, triangles):
    """unit float64 normals of the faces (for the flat-shading figures)"""
    _, _, c, _, _ = faces(vertices, triangles)
    return c / _norm(c)[:, None]


def worst_angle_deg(normals, directions):
    """the largest angle, in degrees, between rows of unit vectors (float64 arithmetic, atan2 of cross and dot: exact near zero)"""
    a, b = np.asarray(normals, np.float64), np.asarray(directions, np.float64)
    return float(np.degrees(np.arctan2(_norm(_cross(a, b)), (a * b).sum(1))).max())


# ---- meshes of the tests --------------------------------------------------------------------------------------------------------------------
def cube():
    """the cube [-1, 1]^3 as 12 triangles wound outwards, two per face"""
    v = np.asarray([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)          # index 4 x + 2 y + z (bits)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.asarray([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def fan(n=4096):
    """n triangles around vertex 0, on a cone so that the hub's normal is not degenerate: one destination for every adder"""
    k = np.arange(n, dtype=np.float64)
    ring = np.stack([np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n), np.full(n, -0.25)], -1)
    v = np.concatenate([np.zeros((1, 3)), ring]).astype(np.float32)
    f = np.stack([np.zeros(n, np.int64), 1 + k.astype(np.int64), 1 + (k.astype(np.int64) + 1) % n], -1).astype(np.int32)
    return v, f


def grid(T, seed=0):
    """a bumpy height field of exactly T triangles (T odd: the last quad keeps one), its rows a little over 100 quads long"""
    nq = (T + 1) // 2
    w = 128
    h = -(-nq // w)
    rg = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h + 1), np.arange(w + 1), indexing='ij')
    v = np.stack([xs, ys, rg.uniform(-0.4, 0.4, xs.shape)], -1).reshape(-1, 3).astype(np.float32)
    q = np.arange(nq)
    a = (q // w) * (w + 1) + q % w
    f = np.stack([np.stack([a, a + 1, a + w + 2], -1), np.stack([a, a + w + 2, a + w + 1], -1)], 1).reshape(-1, 3)[:T]
    return v, f.astype(np.int32)


def spoiled(v, f):
    """(v', f', keep): the mesh v, f with an unreferenced vertex, a NaN vertex used by two faces, a face with an out-of-range index, one with
    a negative index and one with a repeated index appended; keep = the vertices whose normals must have the bits of the clean mesh's"""
    V = len(v)
    v2 = np.concatenate([v, np.asarray([[9, 9, 9], [np.nan, 0, 0]], np.float32)]).astype(np.float32)       # V: unreferenced, V + 1: NaN
    extra = np.asarray([[0, 1, V + 2], [-1, 2, 3], [4, 5, V + 1], [V + 1, 6, 7], [8, 8, 9]], np.int32)
    f2 = np.concatenate([f[:7], extra[:2], f[7:], extra[2:]]).astype(np.int32)
    return v2, f2, np.arange(V)
