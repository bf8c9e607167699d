"""numpy restatement of the ambient-occlusion sample set (nero_ao_rays, include/nero_hip_visibility.h) and of nero_amd.texture.ao_bytes.
Integer-exact up to the square roots and the sine / cosine; float32 throughout, every product and sum rounded on its own."""
import numpy as np

F = np.float32
MAX_RAYS = (1 << 31) - 64


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def bitreverse32(s):
    s = np.asarray(s, dtype=np.uint64)
    out = np.zeros_like(s)
    for k in range(32):
        out |= ((s >> k) & 1) << (31 - k)
    return out


def sample_ab(key, S, seed=0):
    """-> a, b float32 [n, S] in [0, 1): the stratified radius-squared and the radical-inverse angle, rotated per key"""
    key = np.asarray(key).astype(np.int64).astype(np.uint64) & 0xffffffff
    h1 = lowbias32((key * 0x9E3779B9 + (int(seed) & 0xffffffff)) & 0xffffffff)
    h2 = lowbias32((h1 + 0x68E31DA4) & 0xffffffff)
    r1 = ((h1 >> 8).astype(F) * F(2.0 ** -24))[:, None]
    r2 = ((h2 >> 8).astype(F) * F(2.0 ** -24))[:, None]
    s = np.arange(S)
    a = ((s.astype(F) + F(0.5)) / F(S))[None, :] + r1
    a = a - np.floor(a)
    b = (bitreverse32(s).astype(F) * F(2.0 ** -32))[None, :] + r2
    b = b - np.floor(b)
    assert a.dtype == F and b.dtype == F
    return a, b


def frame(n):
    """Duff et al. 2017, branchless: unit normals [n,3] -> tangents t, u [n,3] (float32)"""
    n = np.asarray(n, dtype=F)
    sg = np.copysign(F(1.0), n[:, 2])
    c0 = F(-1.0) / (sg + n[:, 2])
    c1 = n[:, 0] * n[:, 1] * c0
    t = np.stack([F(1.0) + sg * n[:, 0] * n[:, 0] * c0, sg * c1, -sg * n[:, 0]], -1)
    u = np.stack([c1, sg + n[:, 1] * n[:, 1] * c0, -n[:, 1]], -1)
    return t.astype(F), u.astype(F)


def ao_rays(pts, nrm, key, S, seed=0, bias=0.0):
    """-> (rays_o, rays_d) float32 [n S, 3], ray j S + s at that index"""
    pts, nrm = np.asarray(pts, dtype=F), np.asarray(nrm, dtype=F)
    a, b = sample_ab(key, S, seed)
    phi = F(6.283185307179586) * b
    ra = np.sqrt(a)
    x, y, z = ra * np.cos(phi), ra * np.sin(phi), np.sqrt(F(1.0) - a)
    t, u = frame(nrm)
    v = x[..., None] * t[:, None, :] + y[..., None] * u[:, None, :] + z[..., None] * nrm[:, None, :]
    ln = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    d = (v / ln[..., None]).astype(F)
    o = np.broadcast_to((pts + F(bias) * nrm)[:, None, :], d.shape).astype(F)
    return o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()


def ao_bytes(count, S):
    """(510 (S - c) + S) // (2 S): floor(255 (S - c) / S + 1 / 2), linear"""
    c = np.asarray(count).astype(np.int64)
    return ((510 * (S - c) + S) // (2 * S)).astype(np.uint8)


def face_normals(v, f, flip=False):
    v = np.asarray(v, dtype=np.float64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return (-n if flip else n).astype(F)


def fan_disk(radius, height, segments=64):
    """a triangle-fan disk parallel to the xy plane, centred on the z axis -> (verts float32 [segments + 1, 3], tris int32 [segments, 3])"""
    ang = 2 * np.pi * np.arange(segments) / segments
    v = np.concatenate([[[0.0, 0.0, height]], np.stack([radius * np.cos(ang), radius * np.sin(ang), np.full(segments, height)], -1)])
    k = np.arange(segments)
    f = np.stack([np.zeros(segments, np.int64), 1 + k, 1 + (k + 1) % segments], -1)
    return v.astype(F), f.astype(np.int32)
