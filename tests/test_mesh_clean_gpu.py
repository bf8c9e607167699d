"""GPU tier: the connected-component clean-up (nero_amd/csrc/mesh_clean.hip through nero_amd.mesh) against the scipy-based restatement
tests/mesh_clean_ref.py: labels, statistics, compaction, degenerate inputs, determinism, extract_geometry(clean=...), the handoff to the
ray tracer, and the clean-only mode of scripts/extract_mesh.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import mcubes_ref as R
from tests import mesh_clean_ref as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ['sphere', 'torus', 'two_spheres'] + sorted(MR.RANDOM_SHAPES)


def _dev(v, f):
    return (torch.from_numpy(np.array(v, np.float32)).cuda().reshape(-1, 3),
            torch.from_numpy(np.array(f, np.int32)).cuda().reshape(-1, 3))


def _eq(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


def _assert_stats(cc, s, v):
    assert cc.K == s['K']
    assert cc.comp.dtype == torch.int32 and _eq(cc.comp, s['comp']) and _eq(cc.label, MR.labels(s['comp']))
    assert cc.n_verts.dtype == torch.int32 and _eq(cc.n_verts, s['n_verts']) and _eq(cc.n_faces, s['n_faces'])
    assert cc.bbox_min.dtype == torch.float32 and _eq(cc.bbox_min, s['bbox_min']) and _eq(cc.bbox_max, s['bbox_max'])
    assert cc.area.dtype == torch.float64
    # a fixed-order float64 sum of at most 2^20 non-negative terms is within 2^20 2^-53 = 1.2e-10 of any other order
    np.testing.assert_allclose(cc.area.cpu().numpy(), s['area'], rtol=1e-9, atol=0.0)


@pytest.mark.parametrize('name', MESHES, ids=str)
def test_labels_and_statistics_match_the_restatement(name):
    from nero_amd.mesh import connected_components_device
    v, f = MR.mesh_of(name)
    s = MR.ref_stats(name)
    if name in MR.RANDOM_SHAPES:
        assert s['K'] >= MR.RANDOM_SHAPES[name]                        # the case has not degenerated
    _assert_stats(connected_components_device(*_dev(v, f)), s, v)


def test_a_long_thin_component_is_one_component():
    from nero_amd.mesh import connected_components_device
    v, f = MR.mesh_of('tube')
    assert (len(v), len(f)) == (5208, 10412)
    cc = connected_components_device(*_dev(v, f))
    assert cc.K == 1 and int(cc.label.max()) == 0 and int(cc.comp.max()) == 0
    assert cc.n_verts.tolist() == [5208] and cc.n_faces.tolist() == [10412]
    _assert_stats(cc, MR.ref_stats('tube'), v)


def test_partition_does_not_depend_on_the_numbering():
    from nero_amd.mesh import connected_components_device
    v, f = MR.mesh_of((40, 33, 27))
    rg = np.random.default_rng(3)
    new_of_old = rg.permutation(len(v))
    v2 = np.empty_like(v)
    v2[new_of_old] = v
    f2 = new_of_old[f][rg.permutation(len(f))].astype(np.int32)
    f2 = np.stack([np.roll(t, k) for t, k in zip(f2, rg.integers(0, 3, len(f2)))])      # the first vertex of a face moves too
    cc = connected_components_device(*_dev(v2, f2))
    s2 = MR.stats(v2, f2)
    _assert_stats(cc, s2, v2)                                          # canonical under the new numbering
    # the same partition as under the old one: vertices share a component now exactly when they did before
    old = MR.ref_stats((40, 33, 27))
    assert cc.K == old['K']
    now = cc.comp.cpu().numpy()[new_of_old]
    pairs = np.unique(np.stack([old['comp'], now], 1), axis=0)
    assert len(pairs) == old['K'] and len(np.unique(pairs[:, 0])) == old['K'] and len(np.unique(pairs[:, 1])) == old['K']


@pytest.mark.parametrize('rules', [{'keep': 'largest'}, {'keep': 10}, {'min_faces': 30}, {'min_face_ratio': 0.001}, {},
                                   {'keep': 40, 'min_faces': 12}], ids=str)
def test_compaction_matches_the_restatement(rules):
    from nero_amd.mesh import clean_mesh_device
    v, f = MR.mesh_of((40, 33, 27))
    s = MR.ref_stats((40, 33, 27))
    flags = MR.select(s['n_faces'], **rules)
    if rules.get('keep') == 40:                                        # 40 components share the fortieth place: the tie-break decides
        last = np.sort(s['n_faces'])[::-1][39]
        assert (s['n_faces'] == last).sum() > (s['n_faces'][flags] == last).sum() >= 1
    vr, fr, vmap_r = MR.compact(v, f, s['comp'], flags)
    v2, f2, info = clean_mesh_device(*_dev(v, f), **rules)
    assert v2.dtype == torch.float32 and f2.dtype == torch.int32 and info.vmap.dtype == torch.int32
    assert 0 < len(fr) and (len(fr) < len(f) or not rules)
    assert _eq(info.keep, flags) and _eq(info.vmap, vmap_r) and _eq(f2, fr)
    assert v2.shape == vr.shape and _eq(v2.view(torch.int32), vr.view(np.int32))
    _assert_stats(info.components, s, v)


def test_empty_meshes():
    from nero_amd.mesh import clean_mesh_device, connected_components_device
    ev, ef = torch.zeros((0, 3), device='cuda'), torch.zeros((0, 3), dtype=torch.int32, device='cuda')
    cc = connected_components_device(ev, ef)
    assert cc.K == 0 and cc.comp.shape == (0,) and cc.n_faces.shape == (0,) and cc.bbox_min.shape == (0, 3)
    for rules in ({}, {'keep': 'largest'}, {'min_face_ratio': 0.5}):
        v2, f2, info = clean_mesh_device(ev, ef, **rules)
        assert v2.shape == (0, 3) and f2.shape == (0, 3) and info.vmap.shape == (0,) and info.keep.shape == (0,)
    # vertices without a triangle: components of their own without faces, and all of them are dropped
    pv = torch.arange(15, dtype=torch.float32, device='cuda').reshape(5, 3)
    cc = connected_components_device(pv, ef)
    assert cc.K == 5 and cc.comp.tolist() == [0, 1, 2, 3, 4] and cc.n_verts.tolist() == [1] * 5 and cc.n_faces.tolist() == [0] * 5
    assert cc.area.tolist() == [0.0] * 5 and torch.equal(cc.bbox_min, pv) and torch.equal(cc.bbox_max, pv)
    v2, f2, info = clean_mesh_device(pv, ef)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and info.vmap.tolist() == [-1] * 5


def test_unreferenced_duplicate_and_degenerate():
    from nero_amd.mesh import clean_mesh_device
    v = np.arange(21, dtype=np.float32).reshape(7, 3) ** 2
    f = np.array([[1, 2, 4], [4, 2, 1], [1, 2, 4], [5, 6, 6]], np.int32)   # 0 and 3 unreferenced; duplicates; two equal indices
    s = MR.stats(v, f)
    assert s['K'] == 4
    v2, f2, info = clean_mesh_device(*_dev(v, f))
    _assert_stats(info.components, s, v)
    assert info.vmap.tolist() == [-1, 0, 1, -1, 2, 3, 4] and f2.tolist() == [[0, 1, 2], [2, 1, 0], [0, 1, 2], [3, 4, 4]]
    assert _eq(v2, v[[1, 2, 4, 5, 6]])
    v2, f2, info = clean_mesh_device(*_dev(v, f), keep='largest')
    assert info.keep.tolist() == [False, True, False, False] and f2.tolist() == [[0, 1, 2], [2, 1, 0], [0, 1, 2]] and _eq(v2, v[[1, 2, 4]])
    v2, f2, info = clean_mesh_device(*_dev(v, f), min_faces=100)       # a rule that removes everything
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and not info.keep.any() and info.vmap.tolist() == [-1] * 7
    v2, f2, info = clean_mesh_device(*_dev(v, f), keep=0)
    assert v2.shape == (0, 3) and f2.shape == (0, 3)


def test_an_index_out_of_range_raises_and_is_not_followed():
    from nero_amd.mesh import clean_mesh_device, connected_components_device
    v, f = MR.mesh_of((2, 9, 11))
    for bad in (len(v), -1, 2 ** 31 - 1):
        g = f.copy()
        g[len(g) // 2, 1] = bad
        with pytest.raises(ValueError, match='outside'):
            connected_components_device(*_dev(v, g))
        with pytest.raises(ValueError):
            clean_mesh_device(*_dev(v, g), keep='largest')
    torch.cuda.synchronize()
    _assert_stats(connected_components_device(*_dev(v, f)), MR.ref_stats((2, 9, 11)), v)   # the device is as it was


def test_wrong_arguments_raise_type_error():
    from nero_amd.mesh import clean_mesh_device, connected_components_device
    v, f = _dev(*MR.mesh_of((2, 9, 11)))
    for args in ((v.cpu(), f), (v, f.cpu()), (v.double(), f), (v, f.long()), (v[:, :2], f), (v, f[:, :2]), (v.reshape(-1), f),
                 (v.cpu().numpy(), f), (v, None)):
        with pytest.raises(TypeError):
            connected_components_device(*args)
        with pytest.raises(TypeError):
            clean_mesh_device(*args, keep='largest')


def test_two_runs_are_bit_identical():
    from nero_amd.mesh import clean_mesh_device
    u = MR.random_field((64, 50, 45), 7)
    v, f = _dev(*R.marching_cubes(u, 0.0))
    runs = [clean_mesh_device(v, f, keep=25, min_faces=8) for _ in range(2)]
    (v1, f1, i1), (v2, f2, i2) = runs
    assert i1.components.K > 500 and len(f1) > 0
    assert torch.equal(f1, f2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(i1.vmap, i2.vmap)
    assert torch.equal(i1.keep, i2.keep)
    a, b = i1.components, i2.components
    for k in ('label', 'comp', 'n_verts', 'n_faces'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.area.view(torch.int64), b.area.view(torch.int64))
    assert torch.equal(a.bbox_min.view(torch.int32), b.bbox_min.view(torch.int32))
    assert torch.equal(a.bbox_max.view(torch.int32), b.bbox_max.view(torch.int32))


def test_numpy_api_keeps_the_callers_vertices():
    from nero_amd.mesh import clean_mesh
    v, f = MR.mesh_of('two_spheres')
    v64 = v.astype(np.float64) / 3.0                                    # not representable in float32
    v2, f2, info = clean_mesh(v64, f.astype(np.int64), keep='largest')
    vr, fr, vmap = MR.clean(v, f, keep='largest')
    assert v2.dtype == np.float64 and f2.dtype == np.int64
    assert np.array_equal(v2, v64[vmap >= 0]) and np.array_equal(f2, fr) and R.euler_characteristic(v2, f2) == 2


def test_extract_geometry_with_and_without_clean_up():
    from nero_amd import mesh as M
    from bench import BELL, VARIANCE
    from nero_amd.renderer import NeROShapeRenderer
    from nero_amd.synthetic import perturb_state
    torch.manual_seed(6033)
    net = NeROShapeRenderer(dict(BELL), training=False)
    perturb_state(net, VARIANCE)
    net = net.cuda()
    lo, hi = (-1., -1., -1.), (1., 1., 1.)
    # the parent commit's path
    vd, fd = M.marching_cubes_device(net._sdf_grid(lo, hi, 64, 2 ** 21, 1.0), 0.0)
    v0, f0 = M.index_to_world(vd.cpu().numpy(), 64, lo, hi), fd.cpu().numpy().astype(np.int64)
    assert len(f0) > 100
    v, f = net.extract_geometry(resolution=64)
    assert v.dtype == np.float64 and f.dtype == np.int64 and np.array_equal(v, v0) and np.array_equal(f, f0)
    v, f = net.extract_geometry(resolution=64, clean=None)
    assert np.array_equal(v, v0) and np.array_equal(f, f0)
    vc, fc = net.extract_geometry(resolution=64, clean={'keep': 'largest'})
    v1, f1, info = M.clean_mesh(v0, f0, keep='largest')
    assert vc.dtype == np.float64 and fc.dtype == np.int64 and np.array_equal(vc, v1) and np.array_equal(fc, f1)
    s = MR.stats(vd.cpu().numpy(), f0)
    assert len(fc) == int(s['n_faces'].max()) and MR.stats(vc, fc)['K'] == 1


def test_cleaned_mesh_reaches_the_ray_tracer():
    from nero_amd.mesh import clean_mesh_device
    from nero_amd.raytracing import RayTracer
    v, f = MR.mesh_of('two_spheres')
    vd, fd = _dev(v / np.float32(36.0), f)                              # (the tracer reports no hit beyond a distance of 10)
    v2, f2, info = clean_mesh_device(vd, fd, keep='largest')
    assert info.keep.tolist() == [False, True] and len(f2) == 7396
    before, after = RayTracer(vd, fd), RayTracer(v2, f2)
    rg = np.random.default_rng(8)
    n = 512
    d = rg.normal(size=(2 * n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kept_c, gone_c = np.array([50.3, 19.4, 17.9]) / 36.0, np.array([18.2, 19.6, 17.7]) / 36.0
    # towards the kept sphere from its far side of the removed one; across the removed sphere, never towards the kept one
    d[:n, 0] = np.abs(d[:n, 0])
    d[n:, 0] *= 0.1
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    target = np.concatenate([kept_c + rg.uniform(-0.15, 0.15, (n, 3)), gone_c + rg.uniform(-0.15, 0.15, (n, 3))])
    o = target + d * (30.0 / 36.0)
    o, d = torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy((-d).astype(np.float32)).cuda()
    p0, n0, t0 = before.trace(o, d)
    p1, n1, t1 = after.trace(o, d)
    assert bool((t0 < 10).all()) and bool((t1[:n] < 10).all())
    for a, b in ((p0, p1), (n0, n1), (t0, t1)):
        assert torch.equal(a[:n].contiguous().view(torch.int32), b[:n].contiguous().view(torch.int32))
    assert bool((t1[n:] >= 10).all())                                   # the removed sphere no longer occludes


def test_script_cleans_a_ply(tmp_path, capsys):
    from nero_amd.mesh import read_ply, write_ply
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import extract_mesh as E
    finally:
        sys.path.pop(0)
    v, f = MR.mesh_of('two_spheres')
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'sub' / 'out.ply')
    write_ply(src, v, f)
    E.main(['--in', src, '--out', dst, '--keep-largest'])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out['mode'] == 'clean' and out['rules'] == {'keep': 1} and out['kept_components'] == [1]
    assert out['before']['components'] == 2 and [r['n_faces'] for r in out['before']['table']] == [7396, 5420]
    assert out['after']['components'] == 1 and out['after']['n_faces'] == 7396
    v2, f2 = read_ply(dst)
    vr, fr, _ = MR.clean(v, f, keep='largest')
    assert np.array_equal(v2, vr.astype(np.float64)) and np.array_equal(f2, fr)
