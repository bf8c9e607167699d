"""numpy restatement of the projection atlas (nero_amd/csrc/mesh_atlas.hip, include/nero_hip.h nero_mesh_face_adjacency / nero_mesh_chart_*,
nero_amd/texture.py chart_atlas; the definition is DESIGN.md 9.7.1): slow and obvious, the thing the kernels are compared with.  The graph
step is scipy.sparse.csgraph.connected_components over the face graph, an implementation independent of the device's union-find; the
boxes go through the same order-preserving bit images, so that -0 orders below +0 as it does there; the UV arithmetic is float64 with
every operation rounded on its own.  Plus the inputs the atlas tests share."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as _scipy_cc

from tests import mesh_clean_ref as MR

FIXTURES = ['sphere', 'torus', 'two_spheres', 'tube'] + sorted(MR.RANDOM_SHAPES)
SIZE = {(24, 20, 18): 1024, (40, 33, 27): 2048}                      # the smallest power of two at which the scale is not 0 (gutter 4); else 128


# ---- 1-2: valid faces and adjacency -----------------------------------------------------------------------------------------------------
def valid_faces(f, V):
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    inr = ((f >= 0) & (f < V)).all(axis=1)
    return inr & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])


def adjacency(f, V):
    """-> (nbr int32 [T,3], boundary edges, non-manifold edges)"""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    T = len(f)
    nbr = np.full((T, 3), -1, np.int32)
    ok = valid_faces(f, V)
    corner = (3 * np.arange(T)[:, None] + np.arange(3)[None, :])[ok].reshape(-1)         # 3 t + e, ascending
    a = f[ok].reshape(-1)
    b = f[ok][:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    order = np.argsort(key, kind='stable')
    key, corner = key[order], corner[order]
    n = len(key)
    head = np.ones(n, bool)
    head[1:] = key[1:] != key[:-1]
    start = np.nonzero(head)[0]
    length = np.diff(np.append(start, n))
    two = start[length == 2]
    c0, c1 = corner[two], corner[two + 1]
    diff = c0 // 3 != c1 // 3                                          # (always: the three edges of a valid face have three keys)
    flat = nbr.reshape(-1)
    flat[c0[diff]] = c1[diff] // 3
    flat[c1[diff]] = c0[diff] // 3
    return nbr, int((length == 1).sum()), int((length >= 3).sum() + (~diff).sum())


# ---- 3: class ---------------------------------------------------------------------------------------------------------------------------
def face_normals(v, f, ok):
    """(b - a) x (c - a) in float64 from the fp32 vertices, each product and difference rounded on its own; zeros where not ok"""
    p = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    n = np.zeros((len(f), 3))
    g = f[ok]
    with np.errstate(invalid='ignore', over='ignore'):
        u, w = p[g[:, 1]] - p[g[:, 0]], p[g[:, 2]] - p[g[:, 0]]
        n[ok] = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
    return n


def face_classes(v, f):
    """-> int32 [T]: 2 k + (n_k < 0) with k = argmax |n_k| (ties to the lowest axis); 6 = chartless"""
    V = len(np.asarray(v).reshape(-1, 3))
    ok = valid_faces(f, V)
    n = face_normals(v, f, ok)
    good = ok & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
    k = np.argmax(np.abs(np.where(good[:, None], n, 0.0)), axis=1)
    cls = 2 * k + (n[np.arange(len(n)), k] < 0)
    return np.where(good, cls, 6).astype(np.int32)


# ---- 4: charts --------------------------------------------------------------------------------------------------------------------------
def _f2o(x):
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _o2f(k):
    k = np.asarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def charts(v, f):
    """-> dict(nbr, boundary, nonmanifold, face_class, chart int32 [T] (-1 chartless), K, chartless, chart_class int32 [K], n_faces int32
    [K], box float32 [K,4] = (min_p, min_q, max_p, max_q))"""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    T = len(f)
    nbr, nb, nm = adjacency(f, len(v))
    cls = face_classes(v, f)
    t = np.repeat(np.arange(T), 3)
    n = nbr.reshape(-1).astype(np.int64)
    join = (n >= 0) & (cls[t] < 6)
    join[join] &= cls[n[join]] == cls[t[join]]
    chart = np.full(T, -1, np.int32)
    K = 0
    if T:
        _, lab = _scipy_cc(coo_matrix((np.ones(int(join.sum()), np.int8), (t[join], n[join])), shape=(T, T)), directed=False)
        charted = cls < 6
        first = np.full(int(lab.max()) + 1, T, np.int64)
        np.minimum.at(first, lab[charted], np.nonzero(charted)[0])     # the smallest face of each chart (T: a chartless face's own label)
        rank = np.full(len(first), -1, np.int64)
        order = np.argsort(first, kind='stable')
        K = int((first < T).sum())
        rank[order[:K]] = np.arange(K)
        chart = np.where(charted, rank[lab], -1).astype(np.int32)
    cc = np.zeros(K, np.int32)
    cc[chart[chart >= 0]] = cls[chart >= 0]
    lo = np.full((K, 2), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((K, 2), np.uint32)
    has = chart >= 0
    k = (cls[has] >> 1).astype(np.int64)
    corners3 = v[f[has]]                                               # [n, 3 corners, 3 axes]
    rows = np.arange(len(k))[:, None]
    for d, axis in enumerate(((k + 1) % 3, (k + 2) % 3)):
        o = _f2o(corners3[rows, np.arange(3)[None, :], axis[:, None]])  # the images of the projected coordinate of the three corners
        np.minimum.at(lo[:, d], np.repeat(chart[has], 3), o.reshape(-1))
        np.maximum.at(hi[:, d], np.repeat(chart[has], 3), o.reshape(-1))
    return {'nbr': nbr, 'boundary': nb, 'nonmanifold': nm, 'face_class': cls, 'chart': chart, 'K': K, 'chartless': int((chart < 0).sum()),
            'chart_class': cc, 'n_faces': np.bincount(chart[chart >= 0], minlength=K).astype(np.int32),
            'box': np.concatenate([_o2f(lo), _o2f(hi)], 1).reshape(K, 4)}


# ---- 5: UV vertices ---------------------------------------------------------------------------------------------------------------------
def corners(f, chart):
    """-> (ft int32 [T,3], vt_vertex int32 [n_vt], vt_chart int32 [n_vt]): one vt per (chart, vertex) pair in ascending order, then the
    sentinel (-1, -1) every corner of a chartless face points at"""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    chart = np.asarray(chart, dtype=np.int64)
    has = chart >= 0
    key = (chart[has][:, None] << 32) | f[has]
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    ft = np.full(f.shape, len(uniq), np.int32)
    ft[has] = inv.reshape(-1, 3)
    vv, vc = (uniq & 0xFFFFFFFF).astype(np.int32), (uniq >> 32).astype(np.int32)
    if not has.all():
        vv, vc = np.append(vv, np.int32(-1)), np.append(vc, np.int32(-1))
    return ft, vv, vc


# ---- 6-7: rectangles and scale ----------------------------------------------------------------------------------------------------------
def extents(box):
    b = np.asarray(box, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    return b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]


def pack(box, scale, size, gutter):
    """-> rects int64 [K,4] = (ox, oy, w, h), or None when the shelves do not fit"""
    ep, eq = extents(box)
    K = len(ep)
    m = gutter // 2
    wf, hf = np.ceil(ep * scale) + 1, np.ceil(eq * scale) + 1
    if K and not (np.all(wf <= size) and np.all(hf <= size)):          # (also NaN and infinity)
        return None
    w, h = wf.astype(np.int64).tolist(), hf.astype(np.int64).tolist()  # (python ints: the loop below is the slow part)
    rects = [None] * K
    x, y, shelf = m, m, 0
    for c in sorted(range(K), key=lambda c: (-h[c], -w[c], c)):
        if x + w[c] > size - m:
            if x == m:
                return None                                            # wider than the map
            x, y, shelf = m, y + shelf + gutter, 0
        rects[c] = (x, y, w[c], h[c])
        x += w[c] + gutter
        shelf = max(shelf, h[c])
    return np.array(rects, np.int64).reshape(K, 4) if K == 0 or y + shelf <= size - m else None


def min_size(K, gutter):
    """the smallest map that holds K cells of 1 x 1"""
    size = 1
    while pack(np.zeros((K, 4), np.float32), 0.0, size, gutter) is None:
        size += 1
    return size


def choose_scale(box, size, gutter, texels_per_unit=None):
    """-> (scale, rects, bisection steps taken)"""
    if texels_per_unit is not None:
        r = pack(box, float(texels_per_unit), size, gutter)
        if r is None:
            raise ValueError('texels_per_unit does not fit')
        return float(texels_per_unit), r, 0
    ep, eq = extents(box)
    ext = max(float(ep.max()), float(eq.max())) if len(ep) else 0.0
    m = gutter // 2
    hi = max(0.0, (size - 2 * m - 1) / ext) if ext > 0 else 1.0
    r = pack(box, hi, size, gutter)
    if r is not None:
        return hi, r, 0
    if pack(box, 0.0, size, gutter) is None:
        raise ValueError(f'smallest size {min_size(len(ep), gutter)}')
    lo, steps = 0.0, 0
    for _ in range(32):
        mid = 0.5 * (lo + hi)
        steps += 1
        if pack(box, mid, size, gutter) is not None:
            lo = mid
        else:
            hi = mid
    return lo, pack(box, lo, size, gutter), steps


# ---- 8: emission ------------------------------------------------------------------------------------------------------------------------
def emit_uv(v, vt_vertex, vt_chart, chart_class, box, rects, scale, size):
    """-> vt float32 [n_vt, 2]; numpy rounds every float64 operation on its own"""
    v = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    box = np.asarray(box, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    out = np.zeros((len(vt_vertex), 2), np.float32)
    real = np.asarray(vt_vertex) >= 0
    c, i = np.asarray(vt_chart)[real].astype(np.int64), np.asarray(vt_vertex)[real].astype(np.int64)
    cls = np.asarray(chart_class, dtype=np.int64)[c]
    k = cls >> 1
    xp, xq = v[i, (k + 1) % 3], v[i, (k + 2) % 3]
    ox, oy = np.asarray(rects)[c, 0].astype(np.float64), np.asarray(rects)[c, 1].astype(np.float64)
    dp = np.where(cls & 1, box[c, 2] - xp, xp - box[c, 0])
    dq = xq - box[c, 1]
    s = np.float64(scale)
    U = (ox + 0.5) + dp * s
    W = (oy + 0.5) + dq * s
    out[real] = np.stack([U / np.float64(size), W / np.float64(size)], -1).astype(np.float32)
    return out


def atlas(v, f, size, gutter=4, texels_per_unit=None):
    """the whole of chart_atlas -> dict(the fields of charts(), ft, vt_vertex, vt_chart, scale, rects, steps, vt, fill)"""
    out = charts(v, f)
    out['ft'], out['vt_vertex'], out['vt_chart'] = corners(f, out['chart'])
    out['scale'], out['rects'], out['steps'] = choose_scale(out['box'], size, gutter, texels_per_unit)
    out['vt'] = emit_uv(v, out['vt_vertex'], out['vt_chart'], out['chart_class'], out['box'], out['rects'], out['scale'], size)
    out['fill'] = float((out['rects'][:, 2] * out['rects'][:, 3]).sum()) / float(size * size)
    return out


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
_cache = {}


def mesh_of(name):
    """a fixture of tests/mesh_clean_ref.mesh_of, 'box' or 'ramp'; shared read-only"""
    if name in ('box', 'ramp'):
        if name not in _cache:
            _cache[name] = box_mesh() if name == 'box' else helical_ramp()
        return _cache[name]
    return MR.mesh_of(name)


def ref_charts(name):
    key = ('charts', name)
    if key not in _cache:
        _cache[key] = charts(*mesh_of(name))
    return _cache[key]


def ref_atlas(name, size, gutter=4):
    key = ('atlas', name, size, gutter)
    if key not in _cache:
        _cache[key] = atlas(*mesh_of(name), size, gutter)
    return _cache[key]


def box_mesh(sides=(3.0, 2.0, 1.5), origin=(0.25, -1.0, 0.5)):
    """a closed box of twelve outward-wound triangles: six charts of two faces -> (verts float32 [8,3], tris int32 [12,3])"""
    v = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) * np.array(sides) + np.array(origin)
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return v.astype(np.float32), np.array(f, np.int32)


def helical_ramp(turns=2, steps=24, r0=1.0, r1=2.0, pitch=0.5):
    """a ramp that winds `turns` times round the z axis and rises `pitch` per turn: every face looks up (class 4), all are joined edge by
    edge, and the turns lie over each other in the projection along z -> (verts float32 [V,3], tris int32 [T,3])"""
    n = turns * steps
    a = 2 * np.pi * np.arange(n + 1) / steps
    z = pitch * np.arange(n + 1) / steps
    inner = np.stack([r0 * np.cos(a), r0 * np.sin(a), z], -1)
    outer = np.stack([r1 * np.cos(a), r1 * np.sin(a), z], -1)
    v = np.concatenate([inner, outer]).astype(np.float32)
    i = np.arange(n)
    f = np.concatenate([np.stack([i, i + n + 1, i + n + 2], -1), np.stack([i, i + n + 2, i + 1], -1)]).astype(np.int32)
    return v, f


def overlap_brute(vt, ft, h, w):
    """the texel centres covered by more than one triangle, decided texel by texel with exact rational arithmetic on the snapped vertices"""
    from tests import texture_ref as TR
    S = TR.snap(vt, h, w)
    tris = [TR.triangle(S, face) for face in np.asarray(ft).reshape(-1, 3)]
    n = 0
    for y in range(h):
        for x in range(w):
            px, py = 256 * x + 128, 256 * y + 128
            c = 0
            for tri in tris:
                if tri is None:
                    continue
                xs, ys = tri[0], tri[1]
                ins = True
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    dx, dy = xs[b] - xs[a], ys[b] - ys[a]
                    e = dx * (py - ys[a]) - dy * (px - xs[a])
                    ins &= e > 0 or (e == 0 and (dy < 0 or (dy == 0 and dx > 0)))
                c += ins
            n += c > 1
    return n


# ---- coverage properties ----------------------------------------------------------------------------------------------------------------
def chart_map(tri_id, chart):
    return np.where(tri_id >= 0, chart[np.maximum(tri_id, 0)], -1)


def assert_gutter_and_containment(cmap, rects, gutter, factor=1):
    """cmap [h, w]: the chart of every covered texel, -1 elsewhere.  Texels of two charts are more than gutter * factor apart (Chebyshev), and
    each chart's texels lie inside its rectangle scaled by `factor`"""
    cmap = np.asarray(cmap).astype(np.int64)
    h, w = cmap.shape
    yy, xx = np.nonzero(cmap >= 0)
    c = cmap[yy, xx]
    r = np.asarray(rects) * factor
    assert (xx >= r[c, 0]).all() and (xx < r[c, 0] + r[c, 2]).all() and (yy >= r[c, 1]).all() and (yy < r[c, 1] + r[c, 3]).all()
    g = gutter * factor
    big = np.iinfo(np.int64).max
    lo = np.where(cmap >= 0, cmap, big)
    hi = cmap
    pad_lo = np.pad(lo, g, constant_values=big)
    pad_hi = np.pad(hi, g, constant_values=-1)
    mn, mx = lo.copy(), hi.copy()
    for dy in range(2 * g + 1):
        for dx in range(2 * g + 1):
            mn = np.minimum(mn, pad_lo[dy:dy + h, dx:dx + w])
            mx = np.maximum(mx, pad_hi[dy:dy + h, dx:dx + w])
    own = cmap >= 0                                                  # around a covered texel there is no texel of another chart
    assert (mn[own] == cmap[own]).all() and (mx[own] == cmap[own]).all()
