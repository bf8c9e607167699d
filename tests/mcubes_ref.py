"""CPU restatement of the HIP marching cubes (nero_amd/csrc/mcubes.hip, include/nero_hip.h nero_mcubes_*), vectorised numpy, same
conventions and order: corner inside when u < threshold; one vertex per crossing grid edge at a + t e_axis, t = (thr - u_a) / (u_b - u_a) in
float32, ordered by (linear index, axis x<y<z); triangles from the kernel's own case table (parsed out of nero_amd/csrc/mcubes_tables.h),
ordered by (cell's linear index, table position).  Plus the mesh checks and analytic fields the marching-cubes tests share."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES_H = os.path.join(ROOT, 'nero_amd', 'csrc', 'mcubes_tables.h')

# corners (x,y,z offsets) and edges (corner pairs), numbered as in mcubes_tables.h
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
POPC = np.array([bin(x).count('1') for x in range(256)], dtype=np.int64)


def _parse_array(text, name):
    m = re.search(name + r'\s*(\[[^=]*\])\s*=\s*\{(.*?)\};', text, re.S)
    assert m, name
    return [int(x) for x in re.findall(r'-?\d+', re.sub(r'//[^\n]*', '', m.group(2)))]


def load_tables():
    """-> (tri_table int64 [256,16] (-1 padded), tri_count int64 [256]) as the kernel compiles them"""
    text = open(TABLES_H).read()
    tri = np.array(_parse_array(text, 'nero_mcubes_tri_table'), dtype=np.int64).reshape(256, 16)
    cnt = np.array(_parse_array(text, 'nero_mcubes_tri_count'), dtype=np.int64)
    assert cnt.shape == (256,)
    return tri, cnt


TRI_TABLE, TRI_COUNT = load_tables()
# edge -> (corner owning the edge's vertex, axis): the vertex of a cell edge belongs to the grid point at its lower end
EDGE_OWNER = np.array([min(EDGES[e], key=lambda c: CORNERS[c].sum()) for e in range(12)])
EDGE_AXIS = np.array([int(np.argmax(np.abs(CORNERS[a] - CORNERS[b]))) for a, b in EDGES])


def marching_cubes(u, threshold=0.0):
    """u float32 [nx,ny,nz] -> (verts float32 [V,3] index space, tris int32 [T,3])"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    nx, ny, nz = u.shape
    if min(u.shape) < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    thr = np.float32(threshold)
    b = u < thr
    mask = np.zeros(u.shape, np.uint8)
    mask[:-1] |= (b[:-1] != b[1:]).astype(np.uint8)
    mask[:, :-1] |= (b[:, :-1] != b[:, 1:]).astype(np.uint8) << 1
    mask[:, :, :-1] |= (b[:, :, :-1] != b[:, :, 1:]).astype(np.uint8) << 2
    flat, uf = mask.ravel(), u.ravel()
    nv = POPC[flat]
    vbase = np.cumsum(nv) - nv
    V = int(nv.sum())
    verts = np.zeros((V, 3), np.float32)
    strides = (ny * nz, nz, 1)
    for a in range(3):
        idx = np.nonzero(flat & (1 << a))[0]
        vid = vbase[idx] + POPC[flat[idx] & ((1 << a) - 1)]
        ua, ub = uf[idx], uf[idx + strides[a]]
        t = (thr - ua) / (ub - ua)                                   # float32 throughout
        ijk = np.stack(np.unravel_index(idx, u.shape), -1).astype(np.float32)
        ijk[:, a] = ijk[:, a] + t
        verts[vid] = ijk
    cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        cube |= b[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    cube = cube.ravel()
    cells = np.nonzero(TRI_COUNT[cube])[0]                            # in (i, j, k) order = grid linear order
    nt = TRI_COUNT[cube[cells]]
    T = int(nt.sum())
    if T == 0:
        return verts, np.zeros((0, 3), np.int32)
    ci, cj, ck = np.unravel_index(cells, (nx - 1, ny - 1, nz - 1))
    L = (ci * ny + cj) * nz + ck
    rep = np.repeat(np.arange(len(cells)), nt)
    q = np.arange(T) - np.repeat(np.cumsum(nt) - nt, nt)
    tris = np.zeros((T, 3), np.int64)
    for e in range(3):
        edge = TRI_TABLE[cube[cells[rep]], 3 * q + e]
        assert (edge >= 0).all()
        c, a = EDGE_OWNER[edge], EDGE_AXIS[edge]
        owner = L[rep] + CORNERS[c, 0] * strides[0] + CORNERS[c, 1] * strides[1] + CORNERS[c, 2]
        tris[:, e] = vbase[owner] + POPC[flat[owner] & ((1 << a) - 1)]
    return verts, tris.astype(np.int32)


# ---- mesh checks -----------------------------------------------------------------------------------------------------------------------
def crossing_edges(u, threshold=0.0):
    b = np.asarray(u) < np.float32(threshold)
    return int((b[1:] != b[:-1]).sum() + (b[:, 1:] != b[:, :-1]).sum() + (b[:, :, 1:] != b[:, :, :-1]).sum())


def ambiguous_faces(u, threshold=0.0):
    """grid faces with two diagonal corners below and the other two above (Bourke's table may crack there)"""
    b = np.asarray(u) < np.float32(threshold)
    n = 0
    for p, q in ((0, 1), (0, 2), (1, 2)):
        s00 = [slice(None)] * 3
        s00[p], s00[q] = slice(None, -1), slice(None, -1)
        s11, s10, s01 = list(s00), list(s00), list(s00)
        s11[p], s11[q] = slice(1, None), slice(1, None)
        s10[p] = slice(1, None)
        s01[q] = slice(1, None)
        a, d, x, y = b[tuple(s00)], b[tuple(s11)], b[tuple(s10)], b[tuple(s01)]
        n += int(((a & d & ~x & ~y) | (~a & ~d & x & y)).sum())
    return n


def closed_oriented_report(f):
    """-> (every undirected edge used by exactly two triangles, in opposite directions, no degenerate triangle, number of edges)"""
    f = np.asarray(f, dtype=np.int64)
    if len(f) == 0:
        return True, 0
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any():
        return False, -1
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    m = int(f.max()) + 1
    fwd = np.sort(a * m + b)
    rev = np.sort(b * m + a)
    unique = len(np.unique(fwd)) == len(fwd)                         # no directed edge twice
    return bool(unique and np.array_equal(fwd, rev)), len(fwd) // 2


def euler_characteristic(v, f):
    ok, n_edges = closed_oriented_report(f)
    assert ok
    return len(v) - n_edges + len(f)


def signed_volume(v, f):
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


# ---- analytic fields (index space; SDFs negative inside) ---------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')


def sphere_field(shape, centre, radius):
    x, y, z = _grid(shape)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32)


def torus_field(shape, centre, R, r):
    x, y, z = _grid(shape)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - R
    return (np.sqrt(q ** 2 + (z - centre[2]) ** 2) - r).astype(np.float32)


def two_spheres_field(shape, c0, r0, c1, r1):
    return np.minimum(sphere_field(shape, c0, r0), sphere_field(shape, c1, r1))


# (name, field, Euler characteristic, analytic volume in voxels^3)
FIXTURES = {
    'sphere': (lambda: sphere_field((56, 56, 56), (27.3, 27.6, 27.8), 20.0), 2, 4.0 / 3.0 * np.pi * 20.0 ** 3),
    'torus': (lambda: torus_field((64, 64, 30), (31.4, 31.7, 14.6), 19.0, 10.0), 0, 2.0 * np.pi ** 2 * 19.0 * 10.0 ** 2),
    'two_spheres': (lambda: two_spheres_field((72, 40, 36), (18.2, 19.6, 17.7), 12.0, (50.3, 19.4, 17.9), 14.0), 4,
                    4.0 / 3.0 * np.pi * (12.0 ** 3 + 14.0 ** 3)),
}
