"""CPU tier of the geometry evaluation (nero_amd/eval_shape.py, nero_amd/csrc/geom_eval.hip): the numpy restatement tests/geom_ref.py against
the reference's recorded outputs (tests/golden/geom_eval.npz, scripts/gen_golden_geom.py), the voxel contract's invariants, the PLY point
reader and the command line's argument handling.  The device is held to geom_ref by tests/test_geom_eval_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import geom_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'geom_eval.npz'))


def ulp_diff(a, b):
    """distance in float32 units in the last place, measured at the larger magnitude"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_back_projection_matches_the_reference_points():
    z = golden()
    n_views = z['poses'].shape[0]
    assert n_views >= 3
    for i in range(n_views):
        got = geom_ref.back_project(z[f'mask_{i}'], z[f'depth_{i}'], z['Ks'][i], z['poses'][i])
        ref = z[f'ref_pts_{i}']
        assert got.shape == ref.shape and got.dtype == np.float32 and len(ref) > 100
        assert ulp_diff(got, ref).max() <= 1.0, (i, ulp_diff(got, ref).max())


def test_back_projection_through_pixel_centres_lies_on_the_sphere():
    """offset 0.5 inverts the projection the depth map was made with; offset 0 (the reference) is half a pixel off"""
    z = golden()
    on = geom_ref.back_project(z['mask_0'], z['depth_0'], z['Ks'][0], z['poses'][0], offset=0.5)
    off = geom_ref.back_project(z['mask_0'], z['depth_0'], z['Ks'][0], z['poses'][0], offset=0.0)
    assert np.abs(np.linalg.norm(on.astype(np.float64), axis=1) - 0.5).max() < 1e-6
    assert np.abs(np.linalg.norm(off.astype(np.float64), axis=1) - 0.5).max() > 1e-3


def test_nearest_dist_matches_the_reference_and_float64():
    z = golden()
    a, b = z['nn_a'], z['nn_b']
    assert a.shape == (20000, 3) and b.shape == (30000, 3)
    for p0, p1, ref in ((a, b, z['nn_ab']), (b, a, z['nn_ba'])):
        got, idx = geom_ref.nearest_dist(p0, p1, return_index=True)
        d64, _ = geom_ref.nearest_dist64(p0, p1)
        assert got.dtype == np.float32 and ref.dtype == np.float32
        # each of difference, square, sum and square root rounds once in fp32: 4 * 2^-24 of the float64 distance of the same inputs
        assert np.all(np.abs(got - d64) <= 4 * U * d64)
        assert np.all(np.abs(ref - d64) <= 4 * U * d64)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 8 * U * d64)
        pick = np.linalg.norm(p0.astype(np.float64) - p1[idx].astype(np.float64), axis=1)
        assert np.all(pick <= d64 * (1 + 8 * U))
    dup = z['nn_dup']
    assert len(dup) >= 16 and np.all(z['nn_ab'][dup] == 0.0) and np.all(geom_ref.nearest_dist(a[dup], b) == 0.0)


def noisy_sphere(n, seed, radius=0.5, noise=0.004):
    rg = np.random.default_rng(seed)
    p = rg.normal(size=(n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True) * (radius + noise * rg.normal(size=(n, 1)))).astype(np.float32)


def test_voxel_restatement_invariants():
    voxel = 0.01
    p = noisy_sphere(50000, 3)
    out, keys, counts, inv, mean = geom_ref.voxel_down_sample(p, voxel, return_parts=True)
    ijk, o = geom_ref.voxel_indices(p, voxel)
    assert counts.sum() == len(p) and len(out) == len(keys) < len(p)
    assert np.all(np.diff(keys) > 0)                                            # sorted by key, one row per voxel
    vox = np.stack([keys >> 42, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF], 1)
    assert np.array_equal(vox[inv], ijk)                                        # every point contributes to the voxel it lies in
    lo = o + vox * voxel
    assert np.all(mean >= lo - 1e-12) and np.all(mean <= lo + voxel + 1e-12)    # means lie inside their voxel
    perm = np.random.default_rng(4).permutation(len(p))
    out_p, keys_p, counts_p, _, mean_p = geom_ref.voxel_down_sample(p[perm], voxel, return_parts=True)
    assert np.array_equal(keys, keys_p) and np.array_equal(counts, counts_p)
    assert np.abs(mean - mean_p).max() <= 1e-12 * np.abs(mean).max()


def test_voxel_cloud_on_voxel_centres_is_returned_unchanged():
    voxel = 0.25                                                                # (binary fractions: the centres are exact in float32)
    g = np.arange(6, dtype=np.float32) * np.float32(voxel)
    p = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    p = p[np.random.default_rng(5).random(len(p)) < 0.6]
    p[0] = 0.0                                                                  # (keep the minimum corner: the origin is min - voxel / 2)
    out = geom_ref.voxel_down_sample(p, voxel)
    assert np.array_equal(out, p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))])
    assert geom_ref.voxel_down_sample(np.zeros((0, 3), np.float32), voxel).shape == (0, 3)
    one = np.array([[0.3, -0.2, 0.9]], np.float32)
    assert np.array_equal(geom_ref.voxel_down_sample(one, voxel), one)


def test_chamfer_of_two_analytic_spheres_has_the_radial_gap():
    """the known-answer case of the GPU tier, restated on the CPU at a small size: spheres of radius 0.50 and 0.51"""
    from nero_amd.synthetic import look_at_pose
    h = w = 128
    K = np.array([[175.0, 0, w / 2], [0, 175.0, h / 2], [0, 0, 1]])
    clouds = []
    for radius in (0.5, 0.51):
        parts = []
        for cam in ((3.0, 0, 0), (-3.0, 0, 0), (0, 3.0, 0.3), (0, -3.0, 0.3), (0.3, 0, 3.0), (0.3, 0.1, -3.0)):
            pose = look_at_pose(np.array(cam, np.float64)).astype(np.float64)
            depth, mask = geom_ref.sphere_depth(K, pose, h, w, radius)
            parts.append(geom_ref.back_project(mask, depth, K, pose, offset=0.5))
        clouds.append(geom_ref.voxel_down_sample(np.concatenate(parts), 0.01))
    c = geom_ref.chamfer(clouds[0], clouds[1])
    assert 0.01 - 2e-4 <= c <= 0.02, c


@pytest.mark.parametrize('double', [False, True])
@pytest.mark.parametrize('ascii_', [False, True])
def test_ply_point_reader_round_trip(tmp_path, double, ascii_):
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    p = noisy_sphere(257, 6).astype(np.float64 if double else np.float32)
    if double:
        p = p + 1e-12
    path = str(tmp_path / 'pts.ply')
    if ascii_:
        t = 'double' if double else 'float'
        with open(path, 'w') as fh:
            fh.write(f'ply\nformat ascii 1.0\ncomment points only\nelement vertex {len(p)}\nproperty {t} x\nproperty {t} y\nproperty {t} z\n'
                     f'end_header\n')
            for row in p:
                fh.write(' '.join(repr(float(v)) for v in row) + '\n')
    else:
        E.write_ply_points(path, p, double=double)
    got = E.read_ply_points(path)
    assert got.dtype == np.float64 and np.array_equal(got, p.astype(np.float64))
    with pytest.raises(ValueError):                    # the mesh reader keeps rejecting files without faces
        M.read_ply(path)


def test_ply_point_reader_takes_mesh_vertices_and_rejects_garbage(tmp_path):
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    from nero_amd.synthetic import icosphere
    v, f = icosphere(1, 0.5)
    path = str(tmp_path / 'mesh.ply')
    M.write_ply(path, v, f)
    assert np.array_equal(E.read_ply_points(path), v.astype(np.float64))
    bad = str(tmp_path / 'bad.ply')
    open(bad, 'w').write('not a ply\n')
    with pytest.raises(ValueError):
        E.read_ply_points(bad)
    nov = str(tmp_path / 'nov.ply')
    open(nov, 'w').write('ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n')
    with pytest.raises(ValueError):
        E.read_ply_points(nov)


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_shape.py'), *args], capture_output=True, text=True, cwd=ROOT)


def test_cli_argument_handling(tmp_path):
    from nero_amd import eval_shape as E
    assert _cli('--help').returncode == 0
    p = _cli()
    assert p.returncode == 2 and '--pr' in p.stderr                                   # neither procedure chosen
    pts = str(tmp_path / 'a.ply')
    E.write_ply_points(pts, noisy_sphere(10, 7))
    p = _cli('--pr', pts)
    assert p.returncode == 2 and '--gt' in p.stderr                                   # --pr without --gt
    p = _cli('--pr', pts, '--gt', pts, '--mesh', pts)
    assert p.returncode == 2                                                          # both procedures at once
    p = _cli('--mesh', pts, '--views', str(tmp_path / 'views.npz'))
    assert p.returncode == 2 and 'gt' in p.stderr                                     # the synthetic procedure without a ground truth
    p = _cli('--pr', str(tmp_path / 'missing.ply'), '--gt', pts)
    assert p.returncode != 0 and 'missing.ply' in p.stderr


def test_reach_check_and_argument_errors_need_no_device():
    from nero_amd import eval_shape as E
    from nero_amd.synthetic import icosphere, look_at_pose
    v, _ = icosphere(1, 0.5)
    near = look_at_pose(np.array([3.0, 0, 0])).astype(np.float64)
    far = look_at_pose(np.array([9.6, 0, 0])).astype(np.float64)
    E._check_reach(v, near, 'test')
    with pytest.raises(ValueError, match='miss'):
        E._check_reach(v, far, 'test')                                                # 9.6 + the box corner: beyond the tracer's miss distance
    with pytest.raises(ValueError):
        E._cam(np.eye(4), near)
    with pytest.raises(ValueError):
        E.eval_mesh(None, None, [], [], (4, 4))                                       # no ground truth given
