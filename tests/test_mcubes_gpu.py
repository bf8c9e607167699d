"""GPU tier: the HIP marching cubes (nero_amd/csrc/mcubes.hip) against the numpy restatement tests/mcubes_ref.py, its error paths, a 512^3
grid, extract_geometry on the bell fixture model, and the Stage-I -> Stage-II handoff through the BVH tracer."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from tests import mcubes_ref as R

pytestmark = pytest.mark.gpu


def _hip(u, thr=0.0):
    from nero_amd.mesh import marching_cubes_device
    v, f = marching_cubes_device(torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda(), thr)
    return v.cpu().numpy(), f.cpu().numpy()


def _assert_same_mesh(u, thr=0.0):
    v, f = _hip(u, thr)
    vr, fr = R.marching_cubes(u, thr)
    assert v.shape == vr.shape and f.shape == fr.shape
    assert torch.equal(torch.from_numpy(f), torch.from_numpy(fr))
    np.testing.assert_allclose(v, vr, rtol=2.5e-7, atol=1e-7)         # 2 float32 ulps (FMA contraction)
    return v, f


def _random_field(shape, seed, thr):
    rg = np.random.default_rng(seed)
    u = rg.uniform(-1, 1, shape).astype(np.float32)
    u[rg.random(shape) < 0.05] = np.float32(thr)                       # values exactly at the threshold: "above"
    return u


@pytest.mark.parametrize('shape,thr', [((40, 33, 27), 0.0), ((13, 17, 19), 0.25), ((2, 9, 11), 0.0), ((31, 2, 5), -0.3),
                                       ((6, 7, 2), 0.0), ((70, 3, 65), 0.1)])
def test_random_fields_match_reference(shape, thr):
    u = _random_field(shape, sum(shape), thr)
    v, f = _assert_same_mesh(u, thr)
    assert len(v) == R.crossing_edges(u, thr) and len(f) > 0
    if shape == (40, 33, 27):                                          # every case occurs
        b = (u < np.float32(thr)).astype(np.int64)
        cube = sum(b[dx:shape[0] - 1 + dx, dy:shape[1] - 1 + dy, dz:shape[2] - 1 + dz] << c for c, (dx, dy, dz) in enumerate(R.CORNERS))
        assert len(np.unique(cube)) == 256


@pytest.mark.parametrize('name', sorted(R.FIXTURES))
def test_analytic_fields_match_reference(name):
    make, chi, _ = R.FIXTURES[name]
    v, f = _assert_same_mesh(make())
    assert R.euler_characteristic(v, f) == chi and R.signed_volume(v, f) < 0


def test_two_runs_are_bit_identical():
    from nero_amd.mesh import marching_cubes_device
    for u in (_random_field((64, 50, 45), 7, 0.0), R.FIXTURES['torus'][0]()):
        g = torch.from_numpy(u).cuda()
        v1, f1 = marching_cubes_device(g, 0.0)
        v2, f2 = marching_cubes_device(g, 0.0)
        assert torch.equal(f1, f2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 6, 7), (6, 1, 7), (6, 7, 1), (5, 4, 3)])
def test_empty_meshes(shape):
    rg = np.random.default_rng(0)
    for u in (np.ones(shape, np.float32), -np.ones(shape, np.float32), np.zeros(shape, np.float32), rg.uniform(-1, 1, shape).astype(np.float32)):
        v, f = _assert_same_mesh(u, 0.0)
        if min(shape) < 2 or (u >= 0).all() or (u < 0).all():
            assert v.shape == (0, 3) and f.shape == (0, 3)


def _raw_count(u, thr):
    from nero_amd import _lib as L
    from nero_amd import mesh as M
    nx, ny, nz = u.shape
    ws = torch.empty(M.workspace_bytes(u.shape), dtype=torch.uint8, device='cuda')
    tot = torch.full((2,), -1, dtype=torch.int64, device='cuda')
    rc = L.lib.nero_mcubes_count(L.ptr(u), nx, ny, nz, C.c_float(thr), L.ptr(ws), L.ptr(tot), L.stream_ptr())
    assert rc == 0
    V, T = tot.tolist()
    return ws, V, T


def test_capacity_smaller_than_the_count_is_an_error_and_writes_nothing():
    from nero_amd import _lib as L
    u = torch.from_numpy(_random_field((30, 20, 25), 11, 0.0)).cuda()
    nx, ny, nz = u.shape
    ws, V, T = _raw_count(u, 0.0)
    assert V > 0 and T > 0

    def emit(v_cap, t_cap):
        verts = torch.full((V + 64, 3), 7.5, dtype=torch.float32, device='cuda')
        tris = torch.full((T + 64, 3), -5, dtype=torch.int32, device='cuda')
        rc = L.lib.nero_mcubes_emit(L.ptr(u), nx, ny, nz, C.c_float(0.0), L.ptr(ws), L.ptr(verts), v_cap, L.ptr(tris), t_cap,
                                    L.stream_ptr())
        torch.cuda.synchronize()
        return rc, verts, tris
    for v_cap, t_cap in ((V - 1, T), (V, T - 1), (0, 0)):
        rc, verts, tris = emit(v_cap, t_cap)
        assert rc < 0 and b'capacity' in L.lib.nero_last_error()
        assert bool((verts == 7.5).all()) and bool((tris == -5).all())
    rc, verts, tris = emit(V, T)                                       # exact capacities: the mesh, nothing beyond it
    assert rc == 0
    assert bool((verts[V:] == 7.5).all()) and bool((tris[T:] == -5).all()) and bool((tris[:T] >= 0).all())
    vr, fr = R.marching_cubes(u.cpu().numpy(), 0.0)
    assert np.array_equal(tris[:T].cpu().numpy(), fr)


def test_nonfinite_values_do_not_fault():
    u = _random_field((20, 21, 22), 5, 0.0)
    rg = np.random.default_rng(9)
    u[rg.random(u.shape) < 0.03] = np.nan
    u[rg.random(u.shape) < 0.02] = np.inf
    u[rg.random(u.shape) < 0.02] = -np.inf
    v1, f1 = _hip(u)
    v2, f2 = _hip(u)
    assert np.array_equal(f1, f2) and np.array_equal(v1.view(np.int32), v2.view(np.int32))
    assert f1.min() >= 0 and f1.max() < len(v1)


def test_sphere_512():
    from nero_amd import mesh as M
    n, r = 512, 200.0
    ax = torch.arange(n, dtype=torch.float32, device='cuda') - 255.3
    u = torch.sqrt(ax.view(-1, 1, 1) ** 2 + (ax.view(1, -1, 1) + 0.4) ** 2 + (ax.view(1, 1, -1) - 0.2) ** 2) - r
    b = u < 0
    crossing = int((b[1:] != b[:-1]).sum() + (b[:, 1:] != b[:, :-1]).sum() + (b[:, :, 1:] != b[:, :, :-1]).sum())
    cube = torch.zeros((n - 1,) * 3, dtype=torch.int16, device='cuda')
    for c, (dx, dy, dz) in enumerate(R.CORNERS):
        cube |= b[dx:n - 1 + dx, dy:n - 1 + dy, dz:n - 1 + dz].to(torch.int16) << c
    n_tris = int(torch.from_numpy(R.TRI_COUNT).cuda()[cube.long()].sum())
    del cube, b
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    v, f = M.marching_cubes_device(u, 0.0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert len(v) == crossing and len(f) == n_tris
    assert peak <= M.workspace_bytes(u.shape) + 12 * (len(v) + len(f)) + 4096, peak
    # closed and consistently oriented: every directed edge once, and its reverse present
    fl = f.long()
    a = torch.cat([fl[:, 0], fl[:, 1], fl[:, 2]])
    c = torch.cat([fl[:, 1], fl[:, 2], fl[:, 0]])
    fwd, rev = torch.sort(a * len(v) + c).values, torch.sort(c * len(v) + a).values
    assert bool((fwd[1:] != fwd[:-1]).all()) and torch.equal(fwd, rev)
    assert len(v) - len(fwd) // 2 + len(f) == 2


def test_extract_geometry_on_the_bell_model():
    from tests.helpers import build_case_model, load_golden
    net = build_case_model(load_golden('bell_s25000')[1]).cuda()
    v, f = net.extract_geometry(resolution=64)
    u = net.extract_fields(resolution=64)
    vr, fr = R.marching_cubes(u, 0.0)
    assert len(fr) > 100 and v.dtype == np.float64 and f.dtype == np.int64
    assert np.array_equal(f, fr.astype(np.int64))
    scale = 2.0 / 63.0
    world = vr.astype(np.float64) / 63.0 * 2.0 - 1.0                   # network/field.py:1114-1116
    tol = (2.5e-7 * np.abs(vr.astype(np.float64)) + 1e-7) * scale      # the index-space tolerance, carried to the box
    assert (np.abs(v - world) <= tol).all(), np.abs(v - world).max()


def test_numpy_api_matches_device_api():
    import nero_amd.mesh as M
    u = R.FIXTURES['two_spheres'][0]()
    v, f = M.marching_cubes(u.astype(np.float64), 0.0)
    vd, fd = M.marching_cubes_device(torch.from_numpy(u).cuda(), 0.0)
    assert v.dtype == np.float64 and f.dtype == np.int64
    assert np.array_equal(v, vd.cpu().numpy().astype(np.float64)) and np.array_equal(f, fd.cpu().numpy())


def _sphere_mesh(res=64, radius=0.5):
    from nero_amd import mesh as M
    ax = torch.linspace(-1, 1, res, device='cuda')                     # extract_fields' grid
    u = torch.sqrt(ax.view(-1, 1, 1) ** 2 + ax.view(1, -1, 1) ** 2 + ax.view(1, 1, -1) ** 2) - radius
    v, f = M.marching_cubes_device(u, 0.0)
    return M.index_to_world(v.cpu().numpy(), res, (-1, -1, -1), (1, 1, 1)), f.cpu().numpy().astype(np.int64)


def _check_handoff(net, verts, tris, res=64, radius=0.5):
    from oracle.tracer_oracle import trace_bruteforce
    rg = np.random.default_rng(4)
    o = rg.normal(size=(400, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 2.5
    d = -o / np.linalg.norm(o, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    pos, nrm, depth, hit = net.trace(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    pos, nrm, depth, hit = pos.cpu().numpy(), nrm.cpu().numpy(), depth.cpu().numpy()[:, 0].astype(np.float64), hit.cpu().numpy()
    assert hit.all()
    radial = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    dots = (nrm * radial).sum(1)
    assert (dots > 0).all() and np.median(dots) > 0.99                 # outward shading normals
    assert np.abs(depth - (2.5 - radius)).max() < 2.0 / (res - 1)       # within one voxel of the sphere
    pos_o, _, depth_o, _ = trace_bruteforce(np.asarray(verts, np.float32), tris, o, d)
    hit_o = depth_o < 10
    assert (hit != hit_o).sum() <= 2
    good = hit & hit_o & (np.abs(depth - depth_o) < 1e-4)
    assert good.sum() >= len(o) - 2
    assert np.abs(pos[good] - pos_o[good]).max() < 2e-4


def test_stage1_mesh_reaches_the_stage2_renderer(tmp_path, monkeypatch):
    from nero_amd.mesh import write_ply
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import load_golden
    _, meta = load_golden('mat_bell')
    cfg = {'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell'}
    verts, tris = _sphere_mesh()
    net = NeROMaterialRenderer(cfg, mesh=(verts, tris)).cuda()
    _check_handoff(net, verts, tris)
    p = str(tmp_path / 'sphere.ply')
    write_ply(p, verts, tris)
    monkeypatch.setitem(sys.modules, 'trimesh', None)
    net2 = NeROMaterialRenderer({**cfg, 'mesh': p}).cuda()
    _check_handoff(net2, np.asarray(verts, np.float32).astype(np.float64), tris)
