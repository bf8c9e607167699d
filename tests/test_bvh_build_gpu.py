"""GPU tier: the device BVH build (nero_bvh_create_device) against the numpy restatement of the tree (tests/bvh_build_ref.py), bit for bit --
nodes with their padding, triangle records, nero_bvh_info -- and against the host builder's handle; the Python surface on top of it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import bvh_build_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from nero_amd import _lib as L
    return L


def _export(h):
    L = _lib()
    out = [C.c_int() for _ in range(4)]
    L.check(L.lib.nero_bvh_info(h, *[C.byref(x) for x in out]))
    info = tuple(int(x.value) for x in out)
    nodes = np.zeros(max(info[0], 1), R.NODE_DT)
    tris = np.zeros(info[1], R.TRI_DT)
    L.check(L.lib.nero_bvh_export(h, nodes.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p)))
    return info, nodes[:info[0]], tris


def _create(v, f, nT=None, short=0, stream=None):
    """-> (return code, handle); the raw call, so that refusals can be looked at"""
    L = _lib()
    vd, fd = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    nT = len(f) if nT is None else nT
    need = int(L.lib.nero_bvh_build_workspace_bytes(len(v), max(nT, 1)))
    assert need > 0
    ws = torch.empty(need - short, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    h = C.c_void_p()
    sp = C.c_void_p(stream.cuda_stream) if stream is not None else L.stream_ptr()
    rc = L.lib.nero_bvh_create_device(C.c_void_p(vd.data_ptr()), len(v), C.c_void_p(fd.data_ptr()), nT, C.c_void_p(ws.data_ptr()),
                                      C.c_size_t(need - short), sp, C.byref(h))
    torch.cuda.synchronize()
    return rc, h


def _build(v, f, stream=None):
    L = _lib()
    rc, h = _create(v, f, stream=stream)
    L.check(rc)
    try:
        return _export(h)
    finally:
        L.lib.nero_bvh_destroy(h)


def _assert_matches_ref(v, f, ref=None, stream=None):
    ref = R.build(v, f) if ref is None else ref
    info, nodes, tris = _build(v, f, stream)
    assert info == ref['info'], (info, ref['info'])
    if nodes.tobytes() != ref['nodes']:
        bad = np.nonzero(nodes.view(np.uint8).reshape(-1, 64) != np.frombuffer(ref['nodes'], np.uint8).reshape(-1, 64))[0]
        raise AssertionError(f'{len(np.unique(bad))} of {len(nodes)} nodes differ, first {bad[0]}: {nodes[bad[0]]} vs {ref["node_array"][bad[0]]}')
    if tris.tobytes() != ref['tris']:
        bad = np.nonzero((tris.view(np.uint8).reshape(-1, 48) != np.frombuffer(ref['tris'], np.uint8).reshape(-1, 48)).any(1))[0]
        raise AssertionError(f'{len(bad)} of {len(tris)} triangle records differ, first at {bad[0]}')
    return info, nodes, tris


@functools.lru_cache(maxsize=None)
def _ico(subdiv, bumps):
    from nero_amd.synthetic import icosphere
    v, f = icosphere(subdiv, 0.5, bumps)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def _ico6_ref():
    return R.build(*_ico(6, 0.2))


def _S():
    return int(_lib().lib.nero_bvh_build_lds_capacity())


@pytest.mark.parametrize('nT', [1, 2, 4, 5, 8, 9, 10, 11, 19, 20, 80])
def test_edge_sizes(nT):
    """a root that is a leaf, the first node, odd splits"""
    v, f = _ico(1, 0.15)
    assert len(f) == 80
    _assert_matches_ref(v, f[:nT])


@pytest.mark.parametrize('which', ['S-1', 'S', 'S+1', '2S', '2S+1', '4S+3', 'all'])
def test_around_the_lds_capacity(which):
    """sibling ranges that differ by one; ranges handed from the global sorts to the finishing kernel at different levels"""
    S = _S()
    v, f = _ico(6, 0.2)
    assert len(f) == 81920 and 4 * S + 3 < len(f)
    nT = {'S-1': S - 1, 'S': S, 'S+1': S + 1, '2S': 2 * S, '2S+1': 2 * S + 1, '4S+3': 4 * S + 3, 'all': len(f)}[which]
    _assert_matches_ref(v, f[:nT], _ico6_ref() if which == 'all' else None)


def _sphere_mc_mesh():
    from nero_amd.mesh import marching_cubes_device
    from tests.mcubes_ref import sphere_field
    u = torch.from_numpy(sphere_field((24, 24, 24), (11.5, 11.5, 11.5), 8.0)).cuda()
    v, f = marching_cubes_device(u, 0.0)
    return v.cpu().numpy(), f.cpu().numpy()


def _copies(x_zero_signs):
    """64 copies of one triangle, in the plane x = 0 when signs are given (then copy i has x = signs[i] * 0 at every vertex)"""
    n = 64
    tri = np.array([[0.25, 0.0, 0.0], [0.25, 1.0, 0.0], [0.25, 0.0, 1.0]], np.float32)
    v = np.tile(tri[None], (n, 1, 1))
    if x_zero_signs is not None:
        v[:, :, 0] = np.where(np.asarray(x_zero_signs)[:, None] < 0, np.float32(-0.0), np.float32(0.0))
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _flat_mesh():
    n = 23
    xs, ys = np.meshgrid(np.arange(n, dtype=np.float32) * 0.125, np.arange(n, dtype=np.float32) * 0.25, indexing='ij')
    v = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(n * n, np.float32)], 1)
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + n, i + 1], 1), np.stack([i + 1, i + n, i + n + 1], 1)]).astype(np.int32)
    return v, f


@pytest.mark.parametrize('case', ['marching_cubes_sphere', 'copies', 'signed_zero_copies', 'flat'])
def test_tie_cases(case):
    """many equal centroid coordinates: equal keys keep the order they had, -0 and +0 are one key, equal extents take axis 0"""
    if case == 'marching_cubes_sphere':
        v, f = _sphere_mc_mesh()
        _, cen, _, _ = R.triangle_prep(v, f)
        assert len(f) > 1000 and len(np.unique(cen[:, 0])) < len(f) // 2
    elif case == 'copies':
        v, f = _copies(None)
    elif case == 'signed_zero_copies':
        v, f = _copies(np.where(np.arange(64) % 2 == 0, -1, 1))
        assert np.signbit(v[0, 0]) and not np.signbit(v[3, 0])
    else:
        v, f = _flat_mesh()
    ref = R.build(v, f)
    _, _, tris = _assert_matches_ref(v, f, ref)
    if case in ('copies', 'signed_zero_copies'):                       # all extents 0: axis 0, and the order stays the index order
        assert np.array_equal(ref['order'], np.arange(64))
        assert np.array_equal(tris['v0'].view(np.uint32), v[f[:, 0]].view(np.uint32))


def _leaf_contents(nodes, tris, root):
    return [(lo, n, sorted(tris[lo:lo + n].tobytes()[i * 48:(i + 1) * 48] for i in range(n))) for lo, n in R.leaves(nodes, root)]


@pytest.mark.parametrize('subdiv,bumps,n_pts,n_dir', [(3, 0.15, 37, 33), (5, 0.2, 300, 64)])
def test_against_the_host_builder(subdiv, bumps, n_pts, n_dir):
    """the two builders share everything but the order inside a leaf: equal node bytes, equal triangle sets per leaf, and traces that agree
    -- depth and position exactly, the normal on all but at most 2 rays (an exact tie in t inside one leaf)"""
    from nero_amd import _lib as L
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import camera_rays, secondary_rays
    v, f = _ico(subdiv, bumps)
    f = np.ascontiguousarray(f[:, ::-1])
    host, dev = RayTracer(v, f), RayTracer(v, f, build='device')
    ih, nh, th = _export(host._handle())
    idv, nd, td = _export(dev._handle())
    assert ih == idv and nh.tobytes() == nd.tobytes()
    assert _leaf_contents(nh, th, ih[3]) == _leaf_contents(nd, td, idv[3])
    o1, d1 = secondary_rays(v, f, n_pts, n_dir, seed=subdiv)
    o2, d2 = camera_rays(61)
    o, d = torch.cat([o1, o2]), torch.cat([d1, d2])
    assert o.shape[0] % 64 != 0
    for mode in (0, 1):
        res = []
        for rt in (host, dev):
            L.check(L.lib.nero_bvh_set_traversal(rt._handle(), mode))
            res.append([x.clone() for x in rt.trace(o, d)])
        (ph, nrh, dh), (pd, nrd, dd) = res
        assert 0.05 < float((dh < 10).float().mean()) < 0.95
        assert torch.equal(dh, dd) and torch.equal(ph, pd)
        assert int((nrh != nrd).any(-1).sum()) <= 2
    for rt in (host, dev):
        L.check(L.lib.nero_bvh_set_traversal(rt._handle(), 1))


def test_refusals():
    """bad triangles are counted on the device and refused with the count; a valid build straight afterwards is right"""
    L = _lib()
    v, f = _ico(3, 0.15)
    f_bad = f.copy()
    f_bad[17, 1] = len(v)
    rc, h = _create(v, f_bad)
    assert rc == -1 and not h.value and b'1 triangle' in L.lib.nero_last_error()
    v_bad = v.copy()
    v_bad[5, 2] = np.nan
    n_touch = int((f == 5).any(1).sum())
    assert n_touch > 1
    rc, h = _create(v_bad, f)
    assert rc == -1 and not h.value and f'{n_touch} triangle'.encode() in L.lib.nero_last_error()
    _assert_matches_ref(v, f)
    rc, h = _create(v, f, nT=0)
    assert rc == -1 and not h.value
    rc, h = _create(v, f, short=1)
    assert rc == -1 and not h.value
    assert L.lib.nero_bvh_build_workspace_bytes(len(v), 1 << 27) == 0


def test_builds_are_deterministic_and_stream_independent():
    v, f = _ico(6, 0.2)
    ref = _ico6_ref()
    _assert_matches_ref(v, f, ref)
    _assert_matches_ref(v, f, ref)
    _assert_matches_ref(v, f, ref, stream=torch.cuda.Stream())


def _same_trace(a, b, o, d):
    (pa, na, da), (pb, nb, db) = a.trace(o, d), b.trace(o, d)
    assert 0.05 < float((da < 10).float().mean()) < 0.95
    assert torch.equal(da, db) and torch.equal(pa, pb) and int((na != nb).any(-1).sum()) <= 2


def test_raytracer_device_build():
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import camera_rays, secondary_rays
    v, f = _ico(5, 0.2)
    f = np.ascontiguousarray(f[:, ::-1])
    host = RayTracer(v, f)
    from_np = RayTracer(v, f, build='device')
    from_cuda = RayTracer(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), build='device')
    for rt in (from_np, from_cuda):
        assert rt._v.dtype == np.float32 and rt._f.dtype == np.int32 and np.array_equal(rt._v, host._v) and np.array_equal(rt._f, host._f)
    o1, d1 = secondary_rays(v, f, 100, 64, seed=1)
    o2, d2 = camera_rays(61)
    o, d = torch.cat([o1, o2]), torch.cat([d1, d2])
    _same_trace(host, from_np, o, d)
    _same_trace(host, from_cuda, o, d)
    assert from_cuda.info() == from_np.info() == host.info() == dict(zip(('n_nodes', 'n_tris', 'max_depth', 'root'), R.info(len(f))))


def test_material_renderer_device_build():
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import load_golden
    _, meta = load_golden('mat_bell')
    cfg = {'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell'}
    v, f = _ico(3, 0.15)
    f = np.ascontiguousarray(f[:, ::-1])
    assert NeROMaterialRenderer.default_cfg['bvh_build'] == 'host'
    host = NeROMaterialRenderer(cfg, mesh=(v, f)).cuda()
    dev = NeROMaterialRenderer({**cfg, 'bvh_build': 'device'}, mesh=(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda())).cuda()
    assert host.ray_tracer.build == 'host' and dev.ray_tracer.build == 'device'
    assert np.array_equal(dev.mesh_vertices, host.mesh_vertices) and np.array_equal(dev.mesh_triangles, host.mesh_triangles)
    K = torch.tensor([[[40.0, 0.0, 16.0], [0.0, 40.0, 16.0], [0.0, 0.0, 1.0]]], device='cuda')
    pose = torch.tensor([[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.5]]], device='cuda')
    a, b = host._trace_views(K, pose, 32, 32, 'cuda'), dev._trace_views(K, pose, 32, 32, 'cuda')
    hit_a, hit_b = a[5], b[5]
    assert 0 < int(hit_a.sum()) < 32 * 32
    assert torch.equal(hit_a, hit_b) and torch.equal(a[4], b[4])


def test_extract_geometry_stays_on_the_device():
    from bench import BELL, VARIANCE
    from nero_amd.renderer import NeROShapeRenderer
    from nero_amd.synthetic import perturb_state
    torch.manual_seed(6033)
    net = NeROShapeRenderer(dict(BELL), training=False)
    perturb_state(net, VARIANCE)
    net = net.cuda()
    v0, f0 = net.extract_geometry(resolution=48)
    v1, f1 = net.extract_geometry(resolution=48, to_host=False)
    assert v1.is_cuda and f1.is_cuda and v1.dtype == torch.float32 and f1.dtype == torch.int32 and len(f0) > 100
    assert v1.cpu().numpy().tobytes() == v0.astype(np.float32).tobytes()
    assert np.array_equal(f1.cpu().numpy().astype(np.int64), f0)
