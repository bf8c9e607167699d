"""GPU tier of the geometry evaluation (nero_amd/eval_shape.py over nero_amd/csrc/geom_eval.hip): the nearest-neighbour kernel against a float64
brute force and the reference's recorded distances, the voxel down-sample against tests/geom_ref.py bit for bit, depth maps against the
brute-force tracer oracle, back-projection against geom_ref and the reference's recorded points, and the Chamfer procedure end to end.

Tolerances (U = 2^-24, the relative rounding of fp32): a fp32 distance formed as difference, square / fma, sum, square root rounds once in each,
so it is within 4 U d of the float64 distance d of the same float32 inputs; the reference's own values obey the same bound, hence 8 U d between
the two.  Hit distances: the bars of tests/test_tracer.py (0.999-quantile < 2e-5, at most 2 in 6 000 rays beyond 1e-3, 2 hit/miss flips in 6 000
rays)."""
import os

import numpy as np
import pytest
import torch

from tests import geom_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'geom_eval.npz'))


def ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def noisy_sphere(n, seed, radius=0.5, noise=0.004):
    rg = np.random.default_rng(seed)
    p = rg.normal(size=(n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True) * (radius + noise * rg.normal(size=(n, 1)))).astype(np.float32)


def brute64(q, r, chunk=512):
    """float64 brute force on the device: the distance of every q to its nearest r"""
    q64, r64 = q.double(), r.double()
    out = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    for i in range(0, q.shape[0], chunk):
        d2 = None
        for a in range(3):
            d = q64[i:i + chunk, a, None] - r64[None, :, a]
            d2 = d * d if d2 is None else d2.addcmul_(d, d)
        out[i:i + chunk] = d2.min(1).values.sqrt()
    return out


def check_nn(q, r, ref=None, splits=0):
    """the assertions every nearest-neighbour case shares -> (dist, idx) device tensors"""
    from nero_amd import eval_shape as E
    dist, idx = E.nearest_dist(q, r, return_index=True, splits=splits)
    plain = E.nearest_dist(q, r, splits=splits)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and dist.shape == (q.shape[0],) and dist.is_cuda
    assert torch.equal(dist, plain)                                                   # with and without the index: the same distances
    d64 = brute64(q, r)
    err = (dist.double() - d64).abs()
    worst = float((err / d64.clamp_min(1e-300)).max() / U)
    print(f'nn {q.shape[0]} x {r.shape[0]} splits {splits}: worst |dist - d64| / d64 = {worst:.2f} U')
    assert bool((err <= 4 * U * d64).all()), worst
    assert int(idx.min()) >= 0 and int(idx.max()) < r.shape[0]
    pick = (q.double() - r.double()[idx.long()]).norm(dim=1)
    assert bool((pick <= d64 * (1 + 8 * U)).all())
    if ref is not None:
        assert bool(((dist.double() - torch.from_numpy(ref).to(dist.device).double()).abs() <= 8 * U * d64).all())
    return dist, idx


@pytest.mark.parametrize('nq,nr', [(1, 1), (1, 65), (63, 1), (63, 63), (65, 63), (63, 65), (65, 1025), (2049, 2047)])
def test_nearest_dist_small_shapes(nq, nr):
    q = torch.from_numpy(noisy_sphere(nq, 100 + nq)).cuda()
    r = torch.from_numpy(noisy_sphere(nr, 200 + nr)).cuda()
    d, i = check_nn(q, r)
    for splits in (1, 2, 3):
        d2, i2 = check_nn(q, r, splits=splits)
        assert torch.equal(d, d2) and torch.equal(i, i2)


def test_nearest_dist_fixture_clouds_against_the_reference():
    from nero_amd import eval_shape as E
    z = golden()
    a, b, dup = z['nn_a'], z['nn_b'], z['nn_dup']
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d_ab, i_ab = check_nn(ta, tb, ref=z['nn_ab'])
    check_nn(tb, ta, ref=z['nn_ba'])
    assert bool((d_ab[torch.from_numpy(dup).cuda()] == 0.0).all())                    # exact duplicates: exactly zero
    assert np.array_equal(b[i_ab.cpu().numpy()[dup]], a[dup])
    # the reference's contract: numpy in, float32 numpy out; batch_size accepted and ignored
    host = E.nearest_dist(a.astype(np.float64), b, 512)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host, d_ab.cpu().numpy())
    hd, hi = E.nearest_dist(a, b, return_index=True)
    assert hi.dtype == np.int64 and np.array_equal(hi, i_ab.cpu().numpy())
    # ties go to the lowest index: every point of b twice
    d2, i2 = E.nearest_dist(ta, torch.cat([tb, tb]), return_index=True)
    assert torch.equal(d2, d_ab) and torch.equal(i2, i_ab)
    # run to run and across launch shapes: bit-identical
    for splits in (0, 1, 7, 30):
        d3, i3 = E.nearest_dist(ta, tb, return_index=True, splits=splits)
        assert torch.equal(d3, d_ab) and torch.equal(i3, i_ab), splits


def test_nearest_dist_50k_by_500k():
    from nero_amd import eval_shape as E
    q = torch.from_numpy(noisy_sphere(50000, 31)).cuda()
    r = torch.from_numpy(noisy_sphere(500000, 32)).cuda()
    d, i = check_nn(q, r)
    d1, i1 = E.nearest_dist(q, r, return_index=True, splits=5)
    assert torch.equal(d, d1) and torch.equal(i, i1)
    # the automatic launch shape fills the chip at the synthetic procedure's size: 256 CUs x 4 workgroups
    assert E.nn_splits(50000, 500000) > 1 and E.nn_splits(50000, 50000) * ((50000 + 2047) // 2048) >= 1024


def test_nearest_dist_empty_sets_and_bad_arguments():
    from nero_amd import _lib as L
    from nero_amd import eval_shape as E
    r = torch.from_numpy(noisy_sphere(10, 1)).cuda()
    none = torch.zeros((0, 3), device='cuda')
    d, i = E.nearest_dist(none, r, return_index=True)
    assert d.shape == (0,) and i.shape == (0,)
    assert E.nearest_dist(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ValueError):
        E.nearest_dist(r, none)
    ws = torch.empty(4096, dtype=torch.uint8, device='cuda')
    out = torch.empty(10, device='cuda')
    rc = L.lib.nero_nn_dist(L.ptr(r), 10, L.ptr(r), 0, L.ptr(ws), 0, L.ptr(out), None, L.stream_ptr())
    assert rc == -1 and b'nr = 0' in L.lib.nero_last_error()                          # NERO_ERR_ARG
    assert L.lib.nero_nn_dist(L.ptr(r), 10, L.ptr(r), 1 << 31, L.ptr(ws), 0, L.ptr(out), L.ptr(ws), L.stream_ptr()) == -3      # int32 indices
    with pytest.raises(ValueError):
        E.nearest_dist(r, r, splits=5000)
    with pytest.raises(ValueError):
        E.nearest_dist(np.zeros((4, 2)), r)


# ---- voxel down-sample ---------------------------------------------------------------------------------------------------------------------
def test_voxel_down_sample_is_bit_identical_to_the_restatement():
    from nero_amd import eval_shape as E
    p = noisy_sphere(200000, 41)
    ref = geom_ref.voxel_down_sample(p, 0.01)
    got = E.voxel_down_sample(torch.from_numpy(p).cuda(), 0.01)
    assert got.is_cuda and got.dtype == torch.float32 and 10000 < len(ref) < len(p)
    assert got.shape == ref.shape and np.array_equal(got.cpu().numpy(), ref)
    host = E.voxel_down_sample(p.astype(np.float64), 0.01)                              # numpy in -> numpy out
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(host, ref)
    again = E.voxel_down_sample(torch.from_numpy(p).cuda(), 0.01)
    assert torch.equal(got, again)


def test_voxel_down_sample_with_one_crowded_voxel():
    from nero_amd import eval_shape as E
    rg = np.random.default_rng(42)
    crowd = (np.array([0.123, -0.2, 0.31]) + rg.uniform(-0.0005, 0.0005, (12000, 3))).astype(np.float32)
    p = np.concatenate([noisy_sphere(30000, 43), crowd])
    p = p[rg.permutation(len(p))]
    ref, keys, counts, _, _ = geom_ref.voxel_down_sample(p, 0.01, return_parts=True)
    assert counts.max() > 10000
    got = E.voxel_down_sample(torch.from_numpy(p).cuda(), 0.01)
    assert np.array_equal(got.cpu().numpy(), ref)


def test_voxel_down_sample_edge_cases_and_capacity():
    from nero_amd import _lib as L
    from nero_amd import eval_shape as E
    assert E.voxel_down_sample(torch.zeros((0, 3), device='cuda'), 0.01).shape == (0, 3)
    one = torch.tensor([[0.3, -0.2, 0.9]], device='cuda')
    assert torch.equal(E.voxel_down_sample(one, 0.01), one)
    p = torch.from_numpy(noisy_sphere(5000, 44)).cuda()
    ref = geom_ref.voxel_down_sample(p.cpu().numpy(), 0.01)
    assert np.array_equal(E.voxel_down_sample(p, 0.01, capacity=len(ref)).cpu().numpy(), ref)      # exactly enough room
    # one row too few: an error, and nothing written
    need = L.lib.nero_voxel_downsample_workspace_bytes(len(p))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.full((len(ref), 3), -7.0, device='cuda')
    n_out = torch.zeros(1, dtype=torch.int64, device='cuda')
    rc = L.lib.nero_voxel_downsample(L.ptr(p), len(p), 0.01, L.ptr(ws), L.ptr(out), len(ref) - 1, L.ptr(n_out), L.stream_ptr())
    assert rc == -1 and b'capacity' in L.lib.nero_last_error()
    assert int(n_out) == len(ref) and bool((out == -7.0).all())
    with pytest.raises(L.NeroHipError):
        E.voxel_down_sample(p, 0.01, capacity=3)
    with pytest.raises(L.NeroHipError):
        E.voxel_down_sample(p, -1.0)
    wide = torch.tensor([[0.0, 0, 0], [1.0, 0, 0]], device='cuda')                    # 10^7 voxels on x: more than 2^21
    with pytest.raises(NotImplementedError):
        E.voxel_down_sample(wide, 1e-7)


# ---- depth maps and points -------------------------------------------------------------------------------------------------------------------
def rig(n_views=8, radius=3.0):
    """the camera rig of nero_amd.synthetic.synthetic_rays: centres on a sphere of radius 3 at seeded (azimuth, elevation)"""
    from nero_amd.synthetic import look_at_pose
    rg = np.random.default_rng(0)
    az = rg.uniform(0, 2 * np.pi, n_views)
    el = rg.uniform(0.15, 1.2, n_views)
    cams = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1) * radius
    return np.stack([look_at_pose(c) for c in cams], 0).astype(np.float64)


def intrinsics(focal, h, w):
    return np.array([[focal, 0, w / 2], [0, focal, h / 2], [0, 0, 1]], np.float64)


def sagitta(v, f, radius=0.5):
    """radius minus the smallest distance of a face plane from the centre"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return radius - np.abs((n * a).sum(1)).min()


def boundary_of(mask):
    """pixels with a 4-neighbour on the other side of the mask"""
    b = np.zeros_like(mask)
    b[1:, :] |= mask[1:, :] != mask[:-1, :]
    b[:-1, :] |= mask[1:, :] != mask[:-1, :]
    b[:, 1:] |= mask[:, 1:] != mask[:, :-1]
    b[:, :-1] |= mask[:, 1:] != mask[:, :-1]
    return b


def oracle_hit_distances(v, f, o, d, workers=8):
    """oracle.tracer_oracle.trace_bruteforce over chunks of the rays in fresh worker processes (it is one python loop over the rays; the
    workers never touch the GPU)"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    chunks = np.array_split(np.arange(len(o)), workers * 4)
    with ProcessPoolExecutor(workers, mp_context=mp.get_context('spawn')) as ex:
        parts = list(ex.map(geom_ref.trace_chunk, [(v, f, o[c], d[c]) for c in chunks]))
    return np.concatenate(parts)


def test_depth_maps_against_the_bruteforce_tracer():
    from nero_amd import eval_shape as E
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import icosphere
    v, f = icosphere(5, 0.5)
    rt = RayTracer(v, f)
    poses, h, w = rig(), 96, 96
    K = intrinsics(250.0, h, w)
    rays = [E.view_rays(p, K, (h, w)) for p in poses]
    o = torch.cat([r[0] for r in rays]).cpu().numpy()
    d = torch.cat([r[1] for r in rays]).cpu().numpy()
    assert o.shape == (8 * h * w, 3) and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 2e-7
    t_o = oracle_hit_distances(v, f, o, d).reshape(8, h, w)
    n_rays = t_o.size
    flips, dds = 0, []
    for i, pose in enumerate(poses):
        depth, mask = E.render_depth(rt, pose, K, (h, w))
        assert depth.dtype == np.float32 and mask.dtype == bool and depth.shape == mask.shape == (h, w)
        _, _, t = rt.trace(*rays[i])
        t = t.cpu().numpy().reshape(h, w).astype(np.float64)
        assert np.array_equal(mask, t < 10)
        # camera-space z of the hit: the distance along the ray times the cosine to the optical axis
        ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
        dc = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
        z = np.where(mask, t * dc[..., 2] / np.linalg.norm(dc, axis=-1), 0.0).astype(np.float32)
        assert ulp_diff(depth, z)[mask].max() <= 1.0 and np.all(depth[~mask] == 0)
        mask_o = t_o[i] < 10
        assert 0.3 < mask_o.mean() < 0.9
        wrong = mask != mask_o
        flips += int(wrong.sum())
        assert not np.any(wrong & ~boundary_of(mask_o)), np.argwhere(wrong & ~boundary_of(mask_o))
        both = mask & mask_o
        dds.append(np.abs(t[both] - t_o[i][both]))
    dd = np.concatenate(dds)
    print(f'depth: {n_rays} rays, {flips} hit/miss flips, 0.999-quantile {np.quantile(dd, 0.999):.2e}, beyond 1e-3: {int((dd > 1e-3).sum())}')
    assert flips <= 2 * n_rays // 6000, flips
    assert np.quantile(dd, 0.999) < 2e-5 and (dd > 1e-3).sum() <= 2


def test_points_through_pixel_centres_lie_on_the_mesh():
    from nero_amd import eval_shape as E
    from nero_amd.synthetic import icosphere
    v, f = icosphere(5, 0.5)
    s = sagitta(v, f)
    assert 0 < s < 1e-3
    poses, h, w = rig(), 96, 96
    K = intrinsics(250.0, h, w)
    p = E.mesh_eval_points(v, f, poses, [K] * 8, (h, w), voxel_size=None, unproject_offset=0.5)
    norm = p.double().norm(dim=1).cpu().numpy()
    n = len(norm)
    assert n > 0.3 * 8 * h * w
    out = lambda eps: int(((norm < 0.5 - s - eps) | (norm > 0.5 + eps)).sum())
    print(f'on-surface: {n} points, sagitta {s:.2e}, outside the 2e-5 band: {out(2e-5)}, outside the 1e-3 band: {out(1e-3)}')
    assert out(2e-5) <= 0.001 * n and out(1e-3) <= 2 * n / 6000


def test_points_match_the_restatement_and_the_reference():
    from nero_amd import eval_shape as E
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import icosphere
    v, f = icosphere(5, 0.5)
    rt = RayTracer(v, f)
    poses, h, w = rig(), 96, 80
    Ks = [intrinsics(240.0 + 3 * i, h, w) for i in range(8)]
    parts = []
    for i, pose in enumerate(poses):
        depth, mask = E.render_depth(rt, pose, Ks[i], (h, w))
        for off in (0.0, 0.5):
            ref = geom_ref.back_project(mask, depth, Ks[i], pose, offset=off)
            got = E.depth_points(depth, mask, pose, Ks[i], unproject_offset=off).cpu().numpy()
            assert got.shape == ref.shape and len(ref) > 1000
            assert ulp_diff(got, ref).max() <= 1.0, (i, off, ulp_diff(got, ref).max())
        parts.append(E.depth_points(depth, mask, pose, Ks[i]).cpu().numpy())
    # the mesh path (trace + depth + points in one call) gives the same points as render_depth -> depth_points
    cloud = E.mesh_eval_points(v, f, poses, Ks, (h, w), voxel_size=None).cpu().numpy()
    assert np.array_equal(cloud, np.concatenate(parts))
    # the reference's recorded points for the fixture views
    z = golden()
    for i in range(z['poses'].shape[0]):
        got = E.depth_points(z[f'depth_{i}'], z[f'mask_{i}'], z['poses'][i], z['Ks'][i]).cpu().numpy()
        ref = z[f'ref_pts_{i}']
        assert got.shape == ref.shape and ulp_diff(got, ref).max() <= 1.0, (i, ulp_diff(got, ref).max())


def test_render_depth_refuses_geometry_beyond_the_miss_distance():
    from nero_amd import eval_shape as E
    from nero_amd.synthetic import icosphere, look_at_pose
    v, f = icosphere(2, 0.5)
    far = look_at_pose(np.array([0.0, 9.7, 0.0])).astype(np.float64)
    with pytest.raises(ValueError, match='miss'):
        E.render_depth((v, f), far, intrinsics(100.0, 8, 8), (8, 8))
    depth, mask = E.render_depth((v, f), look_at_pose(np.array([0.0, 9.0, 0.0])), intrinsics(100.0, 8, 8), (8, 8))
    assert mask[4, 4] and abs(depth[4, 4] - 8.5) < 0.02


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_eval_mesh_equals_its_stages_and_the_restatement():
    from nero_amd import eval_shape as E
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import icosphere
    v, f = icosphere(4, 0.5)
    poses, h, w = rig(), 128, 128
    Ks = [intrinsics(175.0, h, w)] * 8
    gt = [geom_ref.sphere_depth(Ks[i], poses[i], h, w, 0.51) for i in range(8)]
    gt_d, gt_m = [g[0] for g in gt], [g[1] for g in gt]
    c = E.eval_mesh(v, f, poses, Ks, (h, w), gt_depths=gt_d, gt_masks=gt_m)
    # by hand through the public stages: bit for bit
    rt = RayTracer(v, f)
    maps = [E.render_depth(rt, poses[i], Ks[i], (h, w)) for i in range(8)]
    pr = E.voxel_down_sample(torch.cat([E.depth_points(m[0], m[1], poses[i], Ks[i]) for i, m in enumerate(maps)]), 0.01)
    gp = E.voxel_down_sample(torch.cat([E.depth_points(gt_d[i], gt_m[i], poses[i], Ks[i]) for i in range(8)]), 0.01)
    assert torch.equal(pr, E.mesh_eval_points(v, f, poses, Ks, (h, w))) and torch.equal(gp, E.depth_eval_points(gt_d, gt_m, poses, Ks))
    ch, dist_gt, dist_pr = E.chamfer(pr, gp)
    assert dist_gt.dtype == np.float32 and dist_gt.shape == (len(gp),) and dist_pr.shape == (len(pr),)
    assert c == float((np.mean(E.nearest_dist(gp.cpu().numpy(), pr.cpu().numpy())) + np.mean(E.nearest_dist(pr, gp).cpu().numpy())) / 2) == float(ch)
    assert c == E.eval_mesh(v, f, poses, Ks, (h, w), gt_points=gp)
    # the numpy restatement from the device's depth maps
    pr_ref = geom_ref.voxel_down_sample(np.concatenate([geom_ref.back_project(m[1], m[0], Ks[i], poses[i]) for i, m in enumerate(maps)]), 0.01)
    gp_ref = geom_ref.voxel_down_sample(np.concatenate([geom_ref.back_project(gt_m[i], gt_d[i], Ks[i], poses[i]) for i in range(8)]), 0.01)
    c_ref = geom_ref.chamfer(pr_ref, gp_ref)
    print(f'chamfer {c:.9f}, restatement {c_ref:.9f}, relative difference {abs(c - c_ref) / c_ref / U:.2f} U; {len(pr)} / {len(gp)} points')
    assert abs(c - c_ref) <= 8 * U * c_ref


def test_chamfer_of_the_icosphere_against_a_sphere_one_hundredth_larger():
    """known answer: radius 0.5 (faceted: sagitta s) against analytic depth maps of radius 0.51, points through the pixel centres.  The
    Chamfer distance is the radial gap 0.01, less the faceting s, less the shrinkage of both clouds under voxel means (a chord of one voxel
    diagonal: 3 voxel^2 / (8 r) = 7.5e-5 each), plus at most one voxel diagonal of lateral mismatch."""
    from nero_amd import eval_shape as E
    from nero_amd.synthetic import icosphere
    v, f = icosphere(5, 0.5)
    s = sagitta(v, f)
    poses, h, w = rig(), 512, 512
    Ks = [intrinsics(700.0, h, w)] * 8
    gt = [geom_ref.sphere_depth(Ks[i], poses[i], h, w, 0.51) for i in range(8)]
    c = E.eval_mesh(v, f, poses, Ks, (h, w), gt_depths=[g[0] for g in gt], gt_masks=[g[1] for g in gt], unproject_offset=0.5)
    c0 = E.eval_mesh(v, f, poses, Ks, (h, w), gt_depths=[g[0] for g in gt], gt_masks=[g[1] for g in gt])
    print(f'chamfer through pixel centres {c:.5f} (sagitta {s:.2e}); with the reference offset 0: {c0:.5f}')
    assert 0.01 - s - 2e-4 <= c <= 0.02, c


def test_stage1_mesh_against_itself_has_zero_chamfer(tmp_path):
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    from tests.helpers import build_case_model, load_golden
    net = build_case_model(load_golden('bell_s25000')[1]).cuda()
    v, f = net.extract_geometry(resolution=64)
    assert len(f) > 100
    poses, h, w = rig(), 160, 160
    Ks = [intrinsics(220.0, h, w)] * 8
    pts = E.mesh_eval_points(v, f, poses, Ks, (h, w))
    assert len(pts) > 1000
    assert E.eval_mesh(v, f, poses, Ks, (h, w), gt_points=pts) == 0.0
    # and through the files the command line reads
    path = str(tmp_path / 'stage1.ply')
    M.write_ply(path, v, f)
    assert E.eval_point_clouds(E.read_ply_points(path), E.read_ply_points(path)) == 0.0
