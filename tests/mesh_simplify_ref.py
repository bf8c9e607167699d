"""CPU restatement of the mesh simplification by vertex clustering (nero_amd/csrc/mesh_simplify.hip, include/nero_hip.h
nero_mesh_simplify_*), written in plain numpy from the definition in DESIGN.md and calling nothing of nero_amd.  np.unique and np.add.at do
the grouping (np.add.at adds in ascending index order: vertices in ascending vertex id, contributions in ascending 3 t + corner),
np.linalg.solve the solve.  The placement can be evaluated a second time in np.longdouble: the distance between the two evaluations is the
restatement's own error.  Plus the box fixture and the face-budget search, once by bisection and once by a linear scan."""
import numpy as np

from tests import mcubes_ref as R

LAMBDA = 1e-3
AXIS_LIMIT = 1 << 21
CELL_FACTORS = (1.0, 0.8408964152537145, 0.7071067811865476, 0.5946035575013605)
K_MAX = 80


def default_origin(v):
    """the per-axis float32 minimum, as float64 (exact)"""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    return v.min(axis=0).astype(np.float64)


def longest_side(v):
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    return float((v.max(axis=0).astype(np.float64) - v.min(axis=0).astype(np.float64)).max())


def simplify_cells(D, k):
    return np.float64(D) * 2.0 ** -(k // 4) * CELL_FACTORS[k % 4]


def vertex_keys(v, cell, origin):
    """-> (ijk int64 [V,3], key int64 [V], ok bool [V]); a true float64 division"""
    x = np.asarray(v, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        i = np.floor((x - np.asarray(origin, np.float64)[None, :]) / np.float64(cell))
        ok = (np.isfinite(i) & (i >= 0) & (i < AXIS_LIMIT)).all(axis=1)
    ijk = np.where(ok[:, None], i, 0).astype(np.int64)
    return ijk, (ijk[:, 0] << 42) | (ijk[:, 1] << 21) | ijk[:, 2], ok


def _checked(v, f, cell, origin):
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    cell = float(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f'cell must be positive and finite, got {cell}')
    origin = default_origin(v) if origin is None and len(v) else np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    ijk, key, ok = vertex_keys(v, cell, origin)
    bad_i = int(((f < 0) | (f >= len(v))).any(axis=1).sum())
    bad_v = int((~ok).sum())
    if bad_v or bad_i:
        raise ValueError(f'{bad_v} vertices non-finite or outside the 2^21 cells of an axis, {bad_i} triangles with an index outside')
    return v, f, cell, origin, ijk, key


def survivor_count(v, f, cell, origin=None):
    v, f, cell, origin, ijk, key = _checked(v, f, cell, origin)
    k = key[f]
    return int(((k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])).sum())


def _solve3(M, r):
    """Gaussian elimination without pivoting of symmetric positive definite [n,3,3] systems, in M's dtype (np.longdouble has no LAPACK)"""
    M, r = M.copy(), r.copy()
    for i in range(3):
        for j in range(i + 1, 3):
            q = M[:, j, i] / M[:, i, i]
            M[:, j, :] -= q[:, None] * M[:, i, :]
            r[:, j] -= q * r[:, i]
    x = np.zeros_like(r)
    for i in (2, 1, 0):
        x[:, i] = (r[:, i] - (M[:, i, i + 1:] * x[:, i + 1:]).sum(axis=1)) / M[:, i, i]
    return x


def placement_of(v, f, cid, n_cells, ijk_cell, cell, origin, placement, dtype=np.float64):
    """the positions of all n_cells occupied cells (cid [V] = the cell of each vertex) -> dict(x, cbar, x_unclamped, m_v, m)"""
    p = v.astype(dtype)
    m_v = np.bincount(cid, minlength=n_cells)
    s = np.zeros((n_cells, 3), dtype)
    np.add.at(s, cid, p)
    cbar = s / m_v[:, None].astype(dtype)
    T = len(f)
    m = np.bincount(cid[f].ravel(), minlength=n_cells) if T else np.zeros(n_cells, np.int64)
    if placement == 'mean' or T == 0:
        return {'x': cbar, 'cbar': cbar, 'x_unclamped': cbar, 'm_v': m_v, 'm': m}
    assert placement == 'quadric'
    p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    n = np.cross(p1 - p0, p2 - p0)                                    # unnormalised: area-squared weights
    nn = n[:, :, None] * n[:, None, :]
    A = np.zeros((n_cells, 3, 3), dtype)
    r = np.zeros((n_cells, 3), dtype)
    cc = cid[f]                                                       # [T,3]
    # contributions in the order 3 t + c
    A_terms = np.repeat(nn, 3, axis=0)
    pc = p[f.ravel()]
    nrep = np.repeat(n, 3, axis=0)
    r_terms = nrep * ((nrep * (pc - cbar[cc.ravel()])).sum(axis=1))[:, None]
    np.add.at(A, cc.ravel(), A_terms)
    np.add.at(r, cc.ravel(), r_terms)
    tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    x = cbar.copy()
    go = tr != 0
    if go.any():
        M = A[go] + (dtype(LAMBDA) * (tr[go] / dtype(3)))[:, None, None] * np.eye(3, dtype=dtype)[None]
        d = np.linalg.solve(M, r[go][:, :, None])[:, :, 0] if dtype is np.float64 else _solve3(M, r[go])
        x[go] = cbar[go] + d
    unclamped = x.copy()
    lo = origin.astype(dtype)[None] + ijk_cell.astype(dtype) * dtype(cell)
    hi = origin.astype(dtype)[None] + (ijk_cell + 1).astype(dtype) * dtype(cell)
    x[go] = np.minimum(np.maximum(x[go], lo[go]), hi[go])
    return {'x': x, 'cbar': cbar, 'x_unclamped': unclamped, 'm_v': m_v, 'm': m}


def simplify(v, f, cell, origin=None, placement='quadric', dedup=True, with_longdouble=False):
    """-> dict: verts float64 [V',3], verts32, tris int32 [T',3], cell_key int64 [V'], vmap int32 [V], fmap int32 [T], n_survivors,
    n_duplicates (survivors removed by dedup; 0 without it), cell, origin, and per output vertex ijk, cbar, x_unclamped, m_v (vertices in
    the cell), m (contributions in the cell); with_longdouble: verts_ld, the same placement evaluated in np.longdouble"""
    v, f, cell, origin, ijk, key = _checked(v, f, cell, origin)
    V, T = len(v), len(f)
    ukey, first, cid = np.unique(key, return_index=True, return_inverse=True) if V else (np.zeros(0, np.int64),) * 3
    cid = np.asarray(cid, np.int64).reshape(-1)
    C = len(ukey)
    kf = key[f] if T else np.zeros((0, 3), np.int64)
    surv = (kf[:, 0] != kf[:, 1]) & (kf[:, 1] != kf[:, 2]) & (kf[:, 0] != kf[:, 2])
    used = np.zeros(C, bool)
    used[cid[f[surv]].ravel()] = True
    out_of_cell = np.where(used, np.cumsum(used) - 1, -1)
    vmap = out_of_cell[cid].astype(np.int32) if V else np.zeros(0, np.int32)
    ijk_cell = ijk[first] if V else np.zeros((0, 3), np.int64)
    P = placement_of(v, f, cid, C, ijk_cell, cell, origin, placement) if V else None
    tris = vmap[f[surv]].astype(np.int32).reshape(-1, 3)
    n_surv = int(surv.sum())
    keep = np.ones(n_surv, bool)
    if dedup and n_surv:
        _, first_of = np.unique(np.sort(tris, axis=1), axis=0, return_index=True)
        keep[:] = False
        keep[first_of] = True
    fmap = np.full(T, -1, np.int32)
    fmap[np.nonzero(surv)[0][keep]] = np.arange(int(keep.sum()), dtype=np.int32)
    sel = lambda a: a[used] if V else np.zeros((0,) + a.shape[1:], a.dtype)
    out = {'tris': tris[keep], 'cell_key': ukey[used] if V else ukey, 'vmap': vmap, 'fmap': fmap, 'n_survivors': n_surv,
           'n_duplicates': n_surv - int(keep.sum()), 'cell': cell, 'origin': origin, 'ijk': sel(ijk_cell)}
    if V:
        out.update(verts=P['x'][used], cbar=P['cbar'][used], x_unclamped=P['x_unclamped'][used], m_v=P['m_v'][used], m=P['m'][used])
    else:
        out.update(verts=np.zeros((0, 3)), cbar=np.zeros((0, 3)), x_unclamped=np.zeros((0, 3)), m_v=np.zeros(0, np.int64),
                   m=np.zeros(0, np.int64))
    out['verts32'] = out['verts'].astype(np.float32)
    if with_longdouble and V:
        out['verts_ld'] = placement_of(v, f, cid, C, ijk_cell, cell, origin, placement, dtype=np.longdouble)['x'][used]
    return out


# ---- the face budget --------------------------------------------------------------------------------------------------------------------
def counts_by_k(v, f, origin=None):
    D = longest_side(v)
    return [survivor_count(v, f, simplify_cells(D, k), origin) for k in range(K_MAX + 1)]


def choose_k_scan(counts, N):
    """the largest k with n(k) <= N, by looking at every k; None when there is none"""
    ks = [k for k, n in enumerate(counts) if n <= N]
    return max(ks) if ks else None


def choose_k_bisect(n_of_k, N):
    """the definition: n(0) > N raises; else plain bisection on [0, 80] treating n as non-decreasing.  n_of_k: k -> n(k)"""
    if n_of_k(0) > N:
        raise ValueError(f'target_faces = {N} is below the {n_of_k(0)} faces of the coarsest cell')
    lo, hi = 0, K_MAX + 1                                             # n(lo) <= N; hi is beyond every admissible k
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if n_of_k(mid) <= N:
            lo = mid
        else:
            hi = mid
    return lo


# ---- the box fixture --------------------------------------------------------------------------------------------------------------------
BOX_CENTRE = (19.3, 19.6, 19.1)
BOX_HALF = (11.2, 9.4, 7.7)


def _box_sdf(p, dtype):
    q = np.abs(p - np.asarray(BOX_CENTRE, dtype)) - np.asarray(BOX_HALF, dtype)
    outside = np.sqrt((np.maximum(q, dtype(0)) ** 2).sum(axis=-1, dtype=dtype))
    return (outside + np.minimum(q.max(axis=-1), dtype(0))).astype(dtype)


_box = {}


def box_mesh():
    """the marching-cubes mesh of the float32 box SDF on a 40^3 grid (2066 vertices, 4128 faces), computed once, read-only.  The SDF is
    evaluated in float64 and rounded to float32, as the analytic fields of tests/mcubes_ref.py are: the face y = 29 lies on grid points,
    where a float32 evaluation gives exact zeros and another mesh (1992 vertices)"""
    if not _box:
        g = np.stack(np.meshgrid(*[np.arange(40, dtype=np.float64)] * 3, indexing='ij'), -1)
        v, f = R.marching_cubes(_box_sdf(g, np.float64).astype(np.float32), 0.0)
        v.setflags(write=False)
        f.setflags(write=False)
        _box['m'] = (v, f)
    return _box['m']


def box_surface_distance(x):
    """mean distance of points to the analytic box surface"""
    return float(np.abs(_box_sdf(np.asarray(x, np.float64), np.float64)).mean())
