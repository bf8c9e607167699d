"""The hard cases of the mesh tracer: small seeded meshes and ray sets on which a bounding-volume walk can disagree with the same triangle
test run over every triangle -- rays through vertices and along edges, rays lying in the planes of box faces, direction components that
are zero.  Not a test module: tests/test_tracer_model_cpu.py holds the float32 model of the tracer (oracle/tracer_oracle.py: trace_walk32)
to exhaustive search on them, tests/test_tracer_hard_gpu.py holds the kernels to the model.

Everything is float32 and a function of (name, seed) alone; a mesh has at most 5000 triangles."""
import functools

import numpy as np

from tests import bvh_build_ref as R

N_RAYS, N_RAYS_TINY = 20000, 2000          # per ray set; neither is a multiple of 64 or 256
MISS = 10.0


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def _grid_mesh(x, y, z):
    """x, y, z [n, m] -> the 2 (n-1) (m-1) triangles of the grid"""
    n, m = x.shape
    v = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(np.float32)
    i = (np.arange(n - 1)[:, None] * m + np.arange(m - 1)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + m, i + 1], 1), np.stack([i + 1, i + m, i + m + 1], 1)]).astype(np.int32)
    return v, f


def height_field(kind, cells=48):
    """a cells x cells grid over [-0.5, 0.5]^2: 'smooth' z = 0.1 sin 7x cos 5y, 'noisy' the same + uniform +-0.01, 'flat' z = 0.125"""
    t = (np.arange(cells + 1, dtype=np.float64) / cells - 0.5)
    x, y = np.meshgrid(t, t, indexing='ij')
    z = 0.1 * np.sin(7 * x) * np.cos(5 * y)
    if kind == 'noisy':
        z = z + np.random.default_rng(48).uniform(-0.01, 0.01, z.shape)
    elif kind == 'flat':
        z = np.full_like(x, 0.125)
    else:
        assert kind == 'smooth', kind
    return _grid_mesh(x, y, z)


def mc_sphere():
    """marching cubes of a sphere on a 24^3 grid (tests/mcubes_ref.py), scaled by 1/32 (exact): two coordinates of every vertex lie on
    grid lines, so many vertices, box faces and centroids share coordinates exactly"""
    from tests import mcubes_ref as M
    v, f = M.marching_cubes(M.sphere_field((24, 24, 24), (11.5, 11.5, 11.5), 8.0), 0.0)
    return ((v - np.float32(11.5)) / np.float32(32)).astype(np.float32), f.astype(np.int32)


def box_mesh(k=8, h=0.4):
    """the closed axis-aligned box [-h, h]^3, every face k x k cells: leaf boxes that are flat on each of the three axes"""
    t = np.linspace(-h, h, k + 1)
    a, b = np.meshgrid(t, t, indexing='ij')
    vs, fs, base = [], [], 0
    for axis in range(3):
        for side in (-h, h):
            c = [None, None, None]
            c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = np.full_like(a, side), a, b
            v, f = _grid_mesh(*c)
            vs.append(v); fs.append(f + base); base += len(v)
    v, f = np.concatenate(vs), np.concatenate(fs)
    uniq, inv = np.unique(v, axis=0, return_inverse=True)            # shared vertices along the box's edges
    return uniq.astype(np.float32), inv.reshape(-1)[f].astype(np.int32)


def sliver_strip(n=200, aspect=1e4):
    """2 n triangles of length 1 and width 1 / aspect, side by side, gently curved"""
    y = np.arange(n + 1, dtype=np.float64) / aspect
    x = np.array([-0.5, 0.5])
    xx, yy = np.meshgrid(x, y, indexing='ij')
    return _grid_mesh(xx, yy, 0.05 * np.sin(40 * yy * aspect / n) * xx)


def degenerate_mesh():
    """a 16 x 16 noisy height field; behind it zero-area triangles (a repeated corner; three collinear corners) and an exact duplicate of every
    tenth triangle"""
    v, f = height_field('noisy', 16)
    rg = np.random.default_rng(16)
    i = rg.integers(0, len(v), (40, 2))
    point = np.stack([i[:, 0], i[:, 0], i[:, 1]], 1)                 # two corners the same vertex
    mid = ((v[i[:20, 0]].astype(np.float64) + v[i[:20, 1]]) / 2).astype(np.float32)      # (collinear up to the rounding of the midpoint)
    line = np.stack([i[:20, 0], len(v) + np.arange(20), i[:20, 1]], 1)
    v = np.concatenate([v, mid])
    f = np.concatenate([f, point, line, f[::10]]).astype(np.int32)
    return v, f


def _tie(name):
    from tests import test_bvh_build_gpu as T
    if name == 'copies':
        return T._copies(None)
    if name == 'signed_zero_copies':
        return T._copies(np.where(np.arange(64) % 2 == 0, -1, 1))
    return T._flat_mesh()


MESHES = ('hf_smooth', 'hf_noisy', 'hf_flat', 'mc_sphere', 'box', 'copies', 'signed_zero_copies', 'flat', 'slivers', 'degenerate',
          'nT1', 'nT4', 'nT5', 'nT9')
TINY = ('nT1', 'nT4', 'nT5', 'nT9')


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (verts float32 [nV,3], tris int32 [nT,3])"""
    if name.startswith('hf_'):
        v, f = height_field(name[3:])
    elif name == 'mc_sphere':
        v, f = mc_sphere()
    elif name == 'box':
        v, f = box_mesh()
    elif name in ('copies', 'signed_zero_copies', 'flat'):
        v, f = _tie(name)
    elif name == 'slivers':
        v, f = sliver_strip()
    elif name == 'degenerate':
        v, f = degenerate_mesh()
    else:                                                            # a root that is a leaf (1, 4), one inner node (5), two levels (9)
        v, f = height_field('noisy', 4)
        f = f[np.random.default_rng(4).permutation(len(f))[:int(name[2:])]]
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    assert 1 <= len(f) <= 5000
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def tree(name):
    """the tree of the builders over mesh(name) (tests/bvh_build_ref.py: the device builder's records bit for bit, the host builder's up to the
    order inside a leaf)"""
    return R.build(*mesh(name))


def n_rays(name):
    return N_RAYS_TINY if name in TINY else N_RAYS


# ---- rays --------------------------------------------------------------------------------------------------------------------------------
def _unit32(d):
    """normalised in float32"""
    d = np.asarray(d, np.float32)
    return (d / np.sqrt((d * d).sum(1, dtype=np.float32, keepdims=True))).astype(np.float32)


def _random_unit(rg, n):
    d = rg.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


class _Scene:
    def __init__(self, name):
        self.name = name
        self.v, self.f = mesh(name)
        used = self.v[self.f.reshape(-1)].astype(np.float64)
        self.lo, self.hi = used.min(0), used.max(0)
        self.c = (self.lo + self.hi) / 2
        self.r = max(float(np.linalg.norm(self.hi - self.lo)) / 2, 0.05)
        self.sheet = name.startswith('hf_')

    def origins(self, rg, n):
        """outside the mesh: the height fields are looked at from above (x, y in [-0.6, 0.6], z in [1, 2]), everything else from a shell around it"""
        if self.sheet:
            return np.stack([rg.uniform(-0.6, 0.6, n), rg.uniform(-0.6, 0.6, n), rg.uniform(1, 2, n)], 1)
        return self.c + _random_unit(rg, n) * (self.r * rg.uniform(1.5, 3.0, (n, 1)))

    def vertices(self, rg, n):
        return self.v[self.f[rg.integers(0, len(self.f), n), rg.integers(0, 3, n)]].astype(np.float64)

    def edge_midpoints(self, rg, n):
        t, k = rg.integers(0, len(self.f), n), rg.integers(0, 3, n)
        return (self.v[self.f[t, k]].astype(np.float64) + self.v[self.f[t, (k + 1) % 3]]) / 2

    def interior(self, rg, n):
        """-> points, the triangles they lie in"""
        t = rg.integers(0, len(self.f), n)
        a, b = rg.uniform(size=n), rg.uniform(size=n)
        flip = a + b > 1
        a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
        x = self.v[self.f[t]].astype(np.float64)
        return x[:, 0] + a[:, None] * (x[:, 1] - x[:, 0]) + b[:, None] * (x[:, 2] - x[:, 0]), t

    def face_planes(self, axis):
        """the coordinates of the inner nodes' child-box faces on one axis, with the box they belong to: (value [m], box min [m,3], box max [m,3])"""
        nd = tree(self.name)['node_array']
        if len(nd) == 0:
            return None
        mn, mx = np.concatenate([nd['lmin'], nd['rmin']]), np.concatenate([nd['lmax'], nd['rmax']])
        return np.concatenate([mn[:, axis], mx[:, axis]]), np.concatenate([mn, mn]), np.concatenate([mx, mx])


def _aimed(sc, rg, targets):
    o = sc.origins(rg, len(targets)).astype(np.float32)
    return o, _unit32(targets.astype(np.float32) - o)


def _axis_parallel(sc, rg, n, on_faces):
    """d = +-e_k exactly.  on_faces False: the other two coordinates of the origin are exactly a vertex's.  on_faces True: one of them lies exactly
    on a face of an inner node's child box and the other inside that box's extent -- the ray runs IN the plane of the face, along the box."""
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    k = np.arange(n) % 3
    sign = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0).astype(np.float32)
    tgt = sc.vertices(rg, n).astype(np.float32)
    if on_faces:
        in_plane = (k + 1 + (np.arange(n) // 6) % 2) % 3            # one of the two axes the ray does not run along
        for axis in range(3):
            pl = sc.face_planes(axis)
            if pl is None:                                           # (a root that is a leaf has no boxes: the rays stay on vertices)
                break
            rows = np.nonzero(in_plane == axis)[0]
            j = rg.integers(0, len(pl[0]), len(rows))
            inside = (pl[1][j] + (pl[2][j] - pl[1][j]) * rg.uniform(size=(len(rows), 3))).astype(np.float32)
            tgt[rows] = inside
            tgt[rows, axis] = pl[0][j]
    o[:] = tgt
    far = (sc.r * rg.uniform(1.5, 3.0, n)).astype(np.float32)
    c = sc.c.astype(np.float32)
    o[np.arange(n), k] = c[k] - sign * far
    d[np.arange(n), k] = sign
    return o, d


SPECIAL = (np.float32(0.0), np.float32(-0.0), np.float32(1e-30))


def _zero_components(sc, rg, n):
    """directions with one (first half) and with two (second half) components equal to +0.0, -0.0 or 1e-30, through vertices (even rays) and
    interior points (odd rays): the origin shares those coordinates with its target exactly"""
    tgt = np.where((np.arange(n) % 2 == 0)[:, None], sc.vertices(rg, n), sc.interior(rg, n)[0]).astype(np.float32)
    d = _random_unit(rg, n).astype(np.float32)
    if sc.sheet:
        d[:, 2] = -np.abs(d[:, 2]) - np.float32(0.2)
    a = rg.integers(0, 3, n)
    special = np.asarray(SPECIAL)[rg.integers(0, 3, (n, 2))]
    two = np.arange(n) >= n // 2
    d[np.arange(n), a] = 0
    b = (a + 1 + rg.integers(0, 2, n)) % 3
    d[two, b[two]] = 0
    d = _unit32(d)
    d[np.arange(n), a] = special[:, 0]
    d[two, b[two]] = special[two, 1]
    o = (tgt - d * (sc.r * rg.uniform(1.5, 3.0, (n, 1))).astype(np.float32)).astype(np.float32)
    return o, d


def _secondary(sc, rg, n):
    """Stage II's secondary rays: from a surface point along a direction of the hemisphere on one side of the face, started 1e-5 off the
    surface ALONG THE DIRECTION (o = p + 1e-5 d)"""
    p, t = sc.interior(rg, n)
    x = sc.v[sc.f[t]].astype(np.float64)
    nrm = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
    d = _random_unit(rg, n)
    d = np.where(((d * nrm).sum(1) < 0)[:, None], -d, d)
    d = _unit32(d)
    return (p.astype(np.float32) + np.float32(1e-5) * d).astype(np.float32), d


def _origins_on_geometry(sc, rg, n):
    """origins exactly on a vertex (even rays), and with one coordinate exactly on a box face and the others inside that box (odd rays)"""
    o = sc.vertices(rg, n).astype(np.float32)
    for axis in range(3):
        pl = sc.face_planes(axis)
        if pl is None:
            break
        rows = np.nonzero(np.arange(n) % 6 == 2 * axis + 1)[0]
        j = rg.integers(0, len(pl[0]), len(rows))
        o[rows] = (pl[1][j] + (pl[2][j] - pl[1][j]) * rg.uniform(size=(len(rows), 3))).astype(np.float32)
        o[rows, axis] = pl[0][j]
    return o, _unit32(_random_unit(rg, n))


def _away(sc, rg, n):
    o = sc.origins(rg, n)
    return o.astype(np.float32), _unit32(o - sc.c + 0.3 * sc.r * rg.normal(size=(n, 3)))


def _near_miss_distance(sc, rg, n):
    """an interior point of the mesh at distance 10 +- 1e-4 along the ray"""
    p, _ = sc.interior(rg, n)
    o0 = sc.origins(rg, n)
    d = p - o0
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    t = MISS + rg.uniform(-1e-4, 1e-4, (n, 1))
    o = (p - t * d).astype(np.float32)
    return o, _unit32(p - o.astype(np.float64))


RAY_SETS = ('vertex', 'edge', 'interior', 'axis_vertex', 'axis_face', 'zero_components', 'secondary', 'origin_on_geometry', 'away',
            'near_miss_distance')


@functools.lru_cache(maxsize=None)
def rays(name, ray_set):
    """-> (o, d) float32 [n, 3], read-only"""
    sc = _Scene(name)
    n = n_rays(name)
    rg = np.random.default_rng([MESHES.index(name), RAY_SETS.index(ray_set)])
    if ray_set == 'vertex':
        o, d = _aimed(sc, rg, sc.vertices(rg, n))
    elif ray_set == 'edge':
        o, d = _aimed(sc, rg, sc.edge_midpoints(rg, n))
    elif ray_set == 'interior':
        o, d = _aimed(sc, rg, sc.interior(rg, n)[0])
    elif ray_set in ('axis_vertex', 'axis_face'):
        o, d = _axis_parallel(sc, rg, n, ray_set == 'axis_face')
    else:
        o, d = {'zero_components': _zero_components, 'secondary': _secondary, 'origin_on_geometry': _origins_on_geometry, 'away': _away,
                'near_miss_distance': _near_miss_distance}[ray_set](sc, rg, n)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    assert o.shape == d.shape == (n, 3) and np.isfinite(o).all() and np.isfinite(d).all()
    o.setflags(write=False); d.setflags(write=False)
    return o, d
