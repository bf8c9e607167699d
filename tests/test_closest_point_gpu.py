"""GPU tier of the closest-point query (nero_bvh_closest, RayTracer.closest, eval_shape.point_to_mesh): the kernels
against the float32 exhaustive search of tests/closest_ref.py BIT FOR BIT -- distance, face, weights, point -- through both builders' handles and
both traversal kernels; tests/test_closest_point_cpu.py holds the walk to that search and the search to float64, so the two tiers together
hold the kernels to the geometry.  Independent of the restatement: the closed-form distance to a box, samples of a surface against that
surface and against nearest_dist, and the exact Chamfer distance of a box against its translate."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import closest_ref as CR
from tests import tracer_ref as TR
from tests.test_bvh_build_gpu import _create

pytestmark = pytest.mark.gpu

MESHES = ('hf_noisy', 'mc_sphere', 'box', 'flat', 'slivers', 'degenerate', 'nT1', 'nT9')
RECORD = 1.0         # u D: the tree stores e = fl(v1 - v0); where a test knows the CALLER'S geometry and not the stored one, this stands beside the bounds


def _lib():
    from nero_amd import _lib as L
    return L


class _Tree:
    """a handle of the library over a mesh of tests/tracer_ref.py, from the host or the device builder (the raw calls: RayTracer refuses the
    meshes of fewer than nine triangles)"""

    def __init__(self, name, build):
        L = _lib()
        v, f = TR.mesh(name)
        if build == 'host':
            self.h = C.c_void_p()
            L.check(L.lib.nero_bvh_create(v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p), len(f), C.byref(self.h)))
        else:
            rc, self.h = _create(v.copy(), f.copy())                  # (the cached arrays are read-only)
            L.check(rc)

    def closest(self, pts, max_dist=float('inf'), bary=True, point=True):
        """-> (dist, face, bary or None, point or None) as numpy arrays; pts: float32 numpy [n,3]"""
        L = _lib()
        n = len(pts)
        p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
        dist = torch.full((n,), -7.0, device='cuda')
        face = torch.full((n,), -7, dtype=torch.int32, device='cuda')
        bt = torch.full((n, 2), -7.0, device='cuda') if bary else None
        qt = torch.full((n, 3), -7.0, device='cuda') if point else None
        L.check(L.lib.nero_bvh_closest(self.h, p.data_ptr(), n, max_dist, dist.data_ptr(), face.data_ptr(), L.ptr(bt), L.ptr(qt), L.stream_ptr()))
        torch.cuda.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in (dist, face, bt, qt))

    def close(self):
        _lib().lib.nero_bvh_destroy(self.h)


@functools.lru_cache(maxsize=None)
def _queries(name):
    """every query set of a mesh, one after the other, and what nero_bvh_closest has to write for them: (points [2400,3], (dist, face, bary,
    point)), computed once and shared by the builders and the tests; read-only"""
    pts = np.concatenate([CR.query_set(name, s) for s in CR.SETS])
    res = {k: np.concatenate([CR.reference(name, s)[k] for s in CR.SETS]) for k in ('d2', 'face', 'b1', 'b2', 'slot')}
    want = CR.outputs(res, TR.tree(name)['tri_array'])
    for a in (pts, res['d2']) + want:
        a.setflags(write=False)
    return pts, want, res['d2']


def _same(got, want, what):
    for g, w, field in zip(got, want, ('dist', 'face', 'bary', 'point')):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, field, g.dtype, g.shape)
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = (gb != wb).reshape(len(g), -1).any(1)
        assert not bad.any(), f'{what}: {field} of {int(bad.sum())} of {len(g)} points differs from exhaustive search, first point ' \
                              f'{int(np.argmax(bad))}: {g[int(np.argmax(bad))].tolist()} vs {w[int(np.argmax(bad))].tolist()}'


@pytest.mark.parametrize('build', ['host', 'device'])
@pytest.mark.parametrize('name', MESHES)
def test_kernels_equal_exhaustive_search_bit_for_bit(name, build):
    L = _lib()
    pts, want, _ = _queries(name)
    assert len(pts) % 64 != 0 and len(pts) % 256 != 0
    t = _Tree(name, build)
    try:
        for mode in (0, 1):                                          # the private-stack and the LDS-stack kernel
            L.check(L.lib.nero_bvh_set_traversal(t.h, mode))
            _same(t.closest(pts), want, f'{name}, {build} builder, traversal {mode}')
    finally:
        t.close()


@pytest.mark.parametrize('n', [1, 63, 64, 65, 4097])
def test_every_count_and_every_optional_output_absent_in_turn(n):
    L = _lib()
    pts, want, _ = _queries('hf_noisy')
    idx = (np.arange(n) * 7 + 3) % len(pts)                           # (4097 > 2400: some points come twice)
    t = _Tree('hf_noisy', 'device')
    try:
        for mode in (0, 1):
            L.check(L.lib.nero_bvh_set_traversal(t.h, mode))
            for bary, point in ((True, True), (False, True), (True, False), (False, False)):
                got = t.closest(pts[idx], bary=bary, point=point)
                assert (got[2] is None) == (not bary) and (got[3] is None) == (not point)
                _same(got, tuple(w[idx] for w in want), f'n = {n}, traversal {mode}, bary {bary}, point {point}')
    finally:
        t.close()


@pytest.mark.parametrize('name', ['hf_noisy', 'nT1'])
def test_max_dist(name):
    pts, want, d2 = _queries(name)
    sel = slice(4 * CR.N_POINTS, 7 * CR.N_POINTS)                      # off_0.1, random, far: distances of every size
    pts, want, d2 = pts[sel], tuple(w[sel] for w in want), d2[sel]
    t = _Tree(name, 'host')
    try:
        # below the nearest distance of the set: nothing is found
        md = np.float32(want[0].min()) * np.float32(0.5)
        assert md > 0
        dist, face, bary, point = t.closest(pts, max_dist=float(md))
        assert (face == -1).all() and np.isposinf(dist).all() and not bary.any() and not point.any()
        # max_dist^2 EXACTLY a point's d2: that point is found, and with it exactly the points with d2 <= max_dist^2
        md_all = np.sqrt(d2)
        exact = np.nonzero(md_all * md_all == d2)[0]
        assert len(exact) >= 10, len(exact)
        for k in (exact[np.argsort(d2[exact])[len(exact) // 2]], exact[np.argmin(d2[exact])]):
            r2 = np.float32(md_all[k]) * np.float32(md_all[k])
            assert r2 == d2[k]
            got = t.closest(pts, max_dist=float(md_all[k]))
            near = d2 <= r2
            assert near[k] and got[1][k] == want[1][k] and not near.all()
            assert np.array_equal(got[1] >= 0, near)
            _same(tuple(g[near] for g in got), tuple(w[near] for w in want), f'{name}: within max_dist')
            assert np.isposinf(got[0][~near]).all() and not got[2][~near].any() and not got[3][~near].any()
    finally:
        t.close()


def test_non_finite_coordinates_find_nothing():
    pts, want, _ = _queries('box')
    pts = pts[:200].copy()
    bad = np.arange(0, 200, 3)
    pts[bad, bad % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[(bad // 3) % 3]
    ok = np.ones(200, bool)
    ok[bad] = False
    for build in ('host', 'device'):
        t = _Tree('box', build)
        try:
            got = t.closest(pts)
            assert (got[1][bad] == -1).all() and np.isposinf(got[0][bad]).all() and not got[2][bad].any() and not got[3][bad].any()
            _same(tuple(g[ok] for g in got), tuple(w[:200][ok] for w in want), f'finite points beside non-finite ones ({build})')
        finally:
            t.close()


@pytest.mark.parametrize('build', ['host', 'device'])
def test_raytracer_closest_sorted_unsorted_and_twice(build):
    """RayTracer.closest: sort=True equals sort=False bit for bit, two runs are equal bit for bit, and both are exhaustive search; leading shapes
    and CPU tensors are taken as occluded takes them"""
    from nero_amd.raytracing import RayTracer
    name = 'mc_sphere'
    pts, want, _ = _queries(name)
    rt = RayTracer(*TR.mesh(name), build=build)
    p = torch.from_numpy(pts.copy())
    a = rt.closest(p)                                                # a CPU tensor is moved to the device
    b = rt.closest(p.cuda(), sort=True)
    c = rt.closest(p.cuda())
    for x, y in ((a, b), (a, c)):
        for u, v in zip(x, y):
            assert u.is_cuda and u.dtype == v.dtype and torch.equal(u.view(torch.int32), v.view(torch.int32))
    assert a[0].dtype == torch.float32 and a[1].dtype == torch.int32
    _same(tuple(t.cpu().numpy() for t in b), want, f'RayTracer.closest(sort=True), {build}')
    g = rt.closest(p.cuda().view(8, 300, 3), sort=True)
    assert g[0].shape == (8, 300) and g[1].shape == (8, 300) and g[2].shape == (8, 300, 2) and g[3].shape == (8, 300, 3)
    assert torch.equal(g[3].reshape(-1, 3), a[3])
    e = rt.closest(torch.zeros(0, 3, device='cuda'))
    assert e[0].shape == (0,) and e[3].shape == (0, 3)
    # max_dist through the wrapper: a limit below every distance of the 'far' set
    far = slice(6 * CR.N_POINTS, 7 * CR.N_POINTS)
    assert want[0][far].min() > 0.1
    m = rt.closest(p[far].cuda(), max_dist=float(want[0][far].min()) * 0.5, sort=True)
    assert bool((m[1] == -1).all()) and bool(torch.isinf(m[0]).all())


def _upper_factor(tri_array):
    """EVAL + max(EDGE, interior_factor(s)) with s the SMALLEST sine over the mesh's triangles: the float32-against-float64 bound of
    tests/test_closest_point_cpu.py, for every triangle of the mesh at once"""
    sine, _ = CR.triangle_shape(tri_array, np.arange(len(tri_array)))
    assert sine.min() > 0.4
    return CR.EVAL + max(CR.EDGE, CR.interior_factor(float(sine.min())))


def test_points_outside_a_box_against_the_closed_form():
    """independent of the restatement: outside the closed box [lo, hi]^3 the distance to its surface is |max(lo - p, p - hi, 0)|, in float64
    from the mesh's own float32 corners.  Bound: the CPU test's derived one over the box's triangles (right triangles, s = 0.707), + RECORD"""
    from nero_amd.raytracing import RayTracer
    v, f = TR.mesh('box')
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    pts = np.concatenate([CR.query_set('box', s) for s in ('random', 'far', 'off_0.1')])
    gap = np.maximum(np.maximum(lo - pts, pts - hi), 0.0)
    outside = (gap > 0).any(1)
    assert outside.sum() > 600
    pts, closed = pts[outside], np.sqrt((gap[outside] ** 2).sum(1))
    tri_array = TR.tree('box')['tri_array']
    bound = (_upper_factor(tri_array) + RECORD) * CR.U * CR.scale(pts, tri_array)
    for build in ('host', 'device'):
        dist, face, bary, point = (t.cpu().numpy() for t in RayTracer(v, f, build=build).closest(torch.from_numpy(pts)))
        err = np.abs(dist.astype(np.float64) - closed)
        print(f'box, {build}: max |dist - closed form| = {err.max():.3e}, bound >= {bound.min():.3e}, max ratio {float((err / bound).max()):.3f}')
        assert (err <= bound).all(), (build, float(err.max()), float((err / bound).max()))
        # the reported point lies on the box and at the reported distance
        q = point.astype(np.float64)
        assert (np.abs(np.linalg.norm(pts - q, axis=1) - closed) <= bound).all()
        assert (np.minimum(np.abs(q - lo), np.abs(q - hi)).min(1) <= bound).all() and (q >= lo - bound[:, None]).all() and (q <= hi + bound[:, None]).all()


@functools.lru_cache(maxsize=None)
def _samples(name, n=20000):
    from nero_amd.surface import sample_surface
    v, f = TR.mesh(name)
    return sample_surface(torch.from_numpy(v.copy()).cuda(), torch.from_numpy(f.copy()).cuda(), n, seed=5)


@pytest.mark.parametrize('build', ['host', 'device'])
def test_samples_of_a_surface_lie_on_it_and_nearer_than_its_samples(build):
    """point_to_mesh(samples of A, A) is at most the derived bound -- the samples are float32, so they lie on the surface only to rounding
    (SAMPLE = 4 u |v|: a barycentric mix of three corners) -- and point_to_mesh(x, B) <= nearest_dist(x, samples of B) + bound for every x: a
    sample of B is a point of B's surface up to the same rounding, and nearest_dist rounds its own distance (NN = 4 u D: a difference, three
    squares, two sums, a root)."""
    from nero_amd import eval_shape as E
    A, B = 'hf_noisy', 'box'
    tri_a, tri_b = TR.tree(A)['tri_array'], TR.tree(B)['tri_array']
    sa, sb = _samples(A), _samples(B)
    SAMPLE, NN = 4.0, 4.0
    own = E.point_to_mesh(sa, TR.mesh(A), bvh_build=build)
    assert torch.is_tensor(own) and own.is_cuda and own.dtype == torch.float32 and own.shape == (len(sa),)
    bound_a = (_upper_factor(tri_a) + RECORD + SAMPLE) * CR.U * CR.scale(sa.cpu().numpy(), tri_a)
    print(f'samples of {A} to {A} ({build}): max {float(own.max()):.3e}, bound >= {bound_a.min():.3e}')
    assert (own.cpu().numpy() <= bound_a).all(), float(own.max())
    x = torch.cat([sa, torch.from_numpy(CR.query_set(B, 'random').copy()).cuda(), torch.from_numpy(CR.query_set(B, 'far').copy()).cuda()])
    exact = E.point_to_mesh(x, TR.mesh(B), bvh_build=build).cpu().numpy().astype(np.float64)
    nearest = E.nearest_dist(x, sb).cpu().numpy().astype(np.float64)
    bound_b = (_upper_factor(tri_b) + RECORD + SAMPLE + NN) * CR.U * CR.scale(x.cpu().numpy(), tri_b)
    print(f'{B}: max(exact - nearest sample) = {float((exact - nearest).max()):.3e}, mean floor of the samples {float((nearest - exact).mean()):.3e}')
    assert (exact <= nearest + bound_b).all(), float((exact - nearest).max())
    assert (nearest - exact).mean() > 1e-4                            # and the sample spacing is a floor the exact distance does not have
    # numpy in -> numpy out
    out = E.point_to_mesh(x.cpu().numpy()[:100], TR.mesh(B), bvh_build=build)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(out.astype(np.float64), exact[:100])


def test_eval_meshes_keeps_its_value_without_exact():
    """eval_meshes(exact=False) is what it was: the Chamfer distance of the two sample sets, bit for bit"""
    from nero_amd import eval_shape as E
    from nero_amd.surface import sample_surface
    a, b = TR.mesh('mc_sphere'), TR.mesh('box')
    dev = torch.device('cuda', torch.cuda.current_device())
    cloud = lambda m: sample_surface(E._points(m[0], dev), m[1], 5000, seed=3, stratified=True)
    was = E.eval_point_clouds(cloud(a), cloud(b))
    assert E.eval_meshes(a, b, n=5000, seed=3) == was == E.eval_meshes(a, b, n=5000, seed=3, exact=False)
    assert E.eval_meshes(a, b, n=5000, seed=3, exact=True) < was


def test_exact_chamfer_of_a_box_against_its_translate():
    """A = the closed box [-h, h]^3, B = A moved by t along x, 0 < t <= h.  For a point of A's surface, by the face it lies on (all six of
    area (2h)^2):
      * x = -h: outside B; the nearest point of B is straight ahead on B's face x = -h + t: distance t;
      * x = +h: inside B; the distance to B's surface is the least distance to its six faces, min(t, 2h - t, h - |y|, h - |z|) =
        min(t, u, w) with u, w uniform on [0, h]: mean = int_0^t (1 - s/h)^2 ds = (h/3) (1 - (1 - t/h)^3);
      * the four side faces (y or z = +-h): the point (x, ...) lies ON B's side face when x >= -h + t (distance 0), else -h + t - x from its
        rim: mean = (1/2h) int_0^t s ds = t^2 / (4h).
    Mean over A's surface: m = (t + (h/3)(1 - (1 - t/h)^3) + t^2/h) / 6; B against A is the mirror image, so the exact Chamfer distance is m.
    h = 0.4, t = 0.1: m = 0.03368.  The samples: n = 50000 stratified draws, one per n-th of the area, each stratum within two neighbouring
    triangles of a 32 x 32 grid per face (diameter d <= 2 * 0.8/32 * sqrt(2) = 0.071); the distance is 1-Lipschitz, so a stratum's variance is
    at most d^2/4 and the mean's standard deviation at most d / (2 sqrt(n)) = 1.6e-4.  Tolerance: six of them, 9.5e-4 (3 % of m) -- where the
    nearest-sample Chamfer distance of the same sets is off by its floor of several 1e-3."""
    from nero_amd import eval_shape as E
    h, t, n = 0.4, 0.1, 50000
    v, f = TR.box_mesh(k=32, h=h)
    vb = v.copy()
    vb[:, 0] += np.float32(t)
    m = (t + (h / 3) * (1 - (1 - t / h) ** 3) + t * t / h) / 6
    assert abs(m - 0.03368) < 1e-5
    tol = 6 * (2 * (2 * h / 32) * np.sqrt(2)) / (2 * np.sqrt(n))
    got = E.eval_meshes((v, f), (vb, f), n=n, seed=0, exact=True)
    plain = E.eval_meshes((v, f), (vb, f), n=n, seed=0)
    print(f'exact Chamfer {got:.6f}, closed form {m:.6f}, tolerance {tol:.2e}; nearest-sample Chamfer {plain:.6f}')
    assert abs(got - m) <= tol, (got, m, tol)
    assert got == E.eval_meshes((v, f), (vb, f), n=n, seed=0, exact=True, bvh_build='device')
