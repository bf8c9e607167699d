"""CPU tier of the surface sampler (include/nero_hip_surface.h, nero_amd/surface.py; its binding: tests/test_binding_cpu.py): the entry
points refuse bad arguments before any device call, the limit arithmetic holds at n = 2^31 - 1 and T = 2^31 - 2 under the sanitizers,
and the restatement (tests/surface_ref.py) has the properties the contract promises: the stratified counts, the chi-square of
independent draws, the moments of the barycentric weights, the silence of degenerate triangles, a closed form, and the command lines."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import surface_ref as SR
from tests.helpers import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
T_MAX, N_MAX = 2 ** 31 - 2, 2 ** 31 - 1
SEEDS = (0, 1, 2)
N_IID = 64000


@pytest.fixture(scope='module')
def SF():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import surface
    return surface


@pytest.fixture(scope='module')
def mesh():
    v, f = SR.squashed_icosphere()
    return v, f, SR.surface_cdf(v, f)


@pytest.fixture(scope='module')
def iid(mesh):
    """the independent samples of the three seeds, drawn once"""
    v, f, cd = mesh
    return {s: SR.sample(v, f, cd['cdf'], cd['total'], 0, N_IID, N_IID, s, False) for s in SEEDS}


def _script(name):
    spec = importlib.util.spec_from_file_location('_surface_cli_' + name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_refuse_bad_arguments_without_a_device(SF):
    from nero_amd import _lib as L
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    for T in (0, -1, T_MAX + 1, 2 ** 33 + 7):
        assert lib.nero_surface_cdf_workspace_bytes(T) == 0 and '[1, 2^31 - 2]' in err()
    # nero_surface_cdf(verts, V, tris, T, ws, cdf, info, stream)
    for k in (0, 2, 4, 5, 6):
        a = [p, 8, p, 4, p, p, p, None]
        a[k] = None
        assert lib.nero_surface_cdf(*a) == ERR_ARG and 'nero_surface_cdf: null' in err()
    for V, T in ((0, 4), (8, 0), (-1, 4), (8, -1), (T_MAX + 1, 4), (8, T_MAX + 1), (2 ** 33 + 8, 4), (8, 2 ** 33 + 4)):
        assert lib.nero_surface_cdf(p, V, p, T, p, p, p, None) == ERR_ARG and '[1, 2^31 - 2]' in err()
    assert lib.nero_surface_cdf(p, 8, p, 4, p + 8, p, p, None) == ERR_ARG and 'aligned' in err()
    # nero_surface_sample(verts, V, tris, T, cdf, info, first, n, n_total, seed, stratified, pts, face, bary, normal, stream)
    smp = lambda **kw: lib.nero_surface_sample(*[kw.get(k, d) for k, d in (
        ('verts', p), ('V', 8), ('tris', p), ('T', 4), ('cdf', p), ('info', p), ('first', 0), ('n', 16), ('n_total', 16), ('seed', 0),
        ('stratified', 1), ('pts', p), ('face', None), ('bary', None), ('normal', None), ('stream', None))])
    for k in ('verts', 'tris', 'cdf', 'info', 'pts'):
        assert smp(**{k: None}) == ERR_ARG and 'nero_surface_sample: null' in err()
    for V, T in ((0, 4), (8, 0), (-1, 4), (8, -1), (T_MAX + 1, 4), (8, T_MAX + 1), (2 ** 33 + 8, 4)):
        assert smp(V=V, T=T) == ERR_ARG and '[1, 2^31 - 2]' in err()
    for first, n, n_total in ((-1, 4, 16), (0, -1, 16), (0, 17, 16), (13, 4, 16), (17, 0, 16), (0, 4, -1), (0, 4, N_MAX + 1),
                              (0, N_MAX + 1, N_MAX + 1), (N_MAX, 1, N_MAX), (2 ** 33, 4, 16), (1, 2 ** 63 - 1, 16), (2 ** 63 - 1, 2 ** 63 - 1, 16)):
        assert smp(first=first, n=n, n_total=n_total) == ERR_ARG and 'n_total <= 2^31 - 1' in err(), (first, n, n_total)
    # nothing to do: no device needed, at the limits too, and before any pointer is looked at
    assert smp(n=0) == 0 and smp(first=16, n=0) == 0 and smp(first=N_MAX, n=0, n_total=N_MAX) == 0 and smp(n=0, n_total=0) == 0
    assert smp(n=0, V=T_MAX, T=T_MAX) == 0 and smp(n=0, pts=None, verts=None) == 0


def test_limit_arithmetic_under_the_sanitizer(tmp_path):
    """nero_amd/csrc/surface_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program): at n = 2^31 - 1 and
    T = 2^31 - 2 no index or byte count overflows, and B = min(40, 62 - L) keeps T 2^B <= 2^62"""
    stdout = run_host_program(tmp_path, 'surface_plan_main.cpp')
    rows = [tuple(int(x) for x in ln.split()) for ln in stdout.splitlines() if not ln.startswith('bad')]
    assert len(rows) == 14
    for T, L_, B, blocks, wbytes in rows:
        assert L_ == (T - 1).bit_length() and B == min(40, 62 - L_) == SR.weight_bits(T)
        assert T * 2 ** B <= 2 ** 62 and T * (2 ** B - 1) < 2 ** 62
        assert blocks == -(-T // 256) and wbytes == -(-8 * T // 256) * 256
    assert (T_MAX, 31, 31, 1 << 23, 8 * (T_MAX + 2)) in rows and (2 ** 22, 22, 40, 1 << 14, 1 << 25) in rows


def test_stratified_counts_stay_within_two_of_their_expectation(mesh):
    """systematic sampling: one jittered sample per n-th of the total weight, so a triangle that covers the interval [a, b) of the running sum
    gets between floor and ceil of n (b - a) / total samples, give or take the two ends -- a property, not a statistic"""
    v, f, cd = mesh
    assert len(f) == 320 and 4.0 < cd['a2'].max() / cd['a2'].min() < 4.2
    worst = 0.0
    for n in (1, 63, 64, 65, 1000, 64000):
        for seed in SEEDS:
            s = SR.sample(v, f, cd['cdf'], cd['total'], 0, n, n, seed, True)
            count = np.bincount(s['face'], minlength=len(f))
            dev = np.abs(count - n * cd['w'].astype(np.float64) / cd['total']).max()
            worst = max(worst, float(dev))
            assert dev < 2, (n, seed, dev)
    print('worst |count - n w / total|', worst)


def test_independent_draws_pass_the_chi_square(mesh, iid):
    """chi^2 over the 320 triangles at n = 64000 below 425, the 0.9999 quantile at 319 degrees of freedom"""
    _, f, cd = mesh
    expect = N_IID * cd['w'].astype(np.float64) / cd['total']
    for seed in SEEDS:
        count = np.bincount(iid[seed]['face'], minlength=len(f))
        chi2 = float(((count - expect) ** 2 / expect).sum())
        print('seed', seed, 'chi2', chi2)
        assert chi2 < 425, (seed, chi2)


def test_barycentric_moments_are_those_of_a_uniform_point(iid):
    """uniform on the triangle: E b = 1/3, E b^2 = 1/6, E b1 b2 = 1/12"""
    for seed in SEEDS:
        b = iid[seed]['b']
        np.testing.assert_allclose(b.sum(1), 1.0, atol=1e-15)
        assert b.min() >= 0
        m1, m2, m12 = b.mean(0), (b * b).mean(0), float((b[:, 1] * b[:, 2]).mean())
        print('seed', seed, np.abs(m1 - 1 / 3).max(), np.abs(m2 - 1 / 6).max(), abs(m12 - 1 / 12))
        assert np.abs(m1 - 1 / 3).max() < 0.005 and np.abs(m2 - 1 / 6).max() < 0.004 and abs(m12 - 1 / 12) < 0.002


def test_degenerate_triangles_are_counted_and_never_chosen():
    v, f, good = SR.degenerate_mesh()
    cd = SR.surface_cdf(v, f)
    assert cd['zero_weight'] == len(f) - len(good) and [t for t in range(len(f)) if cd['w'][t] > 0] == list(good)
    assert cd['w'][good[0]] == cd['w'][good[1]] and cd['total'] == 2 * int(cd['w'][good[0]])
    for stratified in (True, False):
        for seed in SEEDS:
            s = SR.sample(v, f, cd['cdf'], cd['total'], 0, 4097, 4097, seed, stratified)
            assert set(s['face'].tolist()) == set(good)
            assert np.isfinite(s['pts']).all() and np.all(s['normal'] == np.asarray([0, 0, 1], np.float32))
    none = SR.surface_cdf(v, f[[0, 2, 3, 6]])
    assert none['total'] == 0 and none['zero_weight'] == 4 and none['e'] == 0 and not none['cdf'].any()
    s = SR.sample(v, f[[0, 2, 3, 6]], none['cdf'], 0, 0, 5, 5)
    assert np.all(s['face'] == -1) and not s['pts'].any()


def test_the_unit_square_in_closed_form():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
    cd = SR.surface_cdf(v, f)
    assert cd['B'] == 40 and cd['e'] == 1 and cd['w'].tolist() == [2 ** 39, 2 ** 39] and cd['total'] == 2 ** 40 and cd['zero_weight'] == 0
    assert cd['area'] == 1.0
    s = SR.sample(v, f, cd['cdf'], cd['total'], 0, 1000, 1000, 5, True)
    assert np.bincount(s['face']).tolist() == [500, 500]
    assert np.all(s['pts'][:, 2] == 0) and s['pts'].min() >= 0 and s['pts'].max() <= 1
    below = s['pts'][:, 1] <= s['pts'][:, 0]                          # triangle 0 lies under the diagonal
    assert np.all(below[s['face'] == 0]) and np.all(s['pts'][s['face'] == 1][:, 1] >= s['pts'][s['face'] == 1][:, 0])
    # the largest doubled area 1.5 times a power of two: e is one above that power, far from either boundary
    cd = SR.surface_cdf(v * np.asarray([1.5, 1, 1], np.float32), f)
    assert cd['a2'].tolist() == [1.5, 1.5] and cd['e'] == 1 and cd['w'].tolist() == [3 * 2 ** 38] * 2 and cd['area'] == 1.5


def test_chunks_of_the_restatement_are_slices_of_the_whole(mesh):
    v, f, cd = mesh
    for stratified in (True, False):
        whole = SR.sample(v, f, cd['cdf'], cd['total'], 0, 4097, 4097, 3, stratified)
        part = SR.sample(v, f, cd['cdf'], cd['total'], 1000, 1000, 4097, 3, stratified)
        for k in ('pts', 'face', 'bary', 'normal'):
            assert np.array_equal(whole[k][1000:2000], part[k])


def test_the_command_lines(tmp_path, SF):
    from nero_amd import eval_shape as E
    from nero_amd import mesh as M
    run = lambda name, *args: subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', name), *args], capture_output=True, text=True, cwd=ROOT)
    p = run('sample_mesh.py', '--help')
    assert p.returncode == 0 and '--iid' in p.stdout
    p = run('eval_shape.py', '--help')
    assert p.returncode == 0 and '--samples' in p.stdout and '--seed' in p.stdout and '--iid' in p.stdout
    rg = np.random.default_rng(3)
    cloud, mesh_path = str(tmp_path / 'cloud.ply'), str(tmp_path / 'mesh.ply')
    pts = rg.normal(size=(10, 3)).astype(np.float32)
    E.write_ply_points(cloud, pts)
    v, f = SR.squashed_icosphere()
    M.write_ply(mesh_path, v, f)
    es = _script('eval_shape')
    assert es.has_faces(mesh_path) and not es.has_faces(cloud)
    a = es.parse(['--pr', cloud, '--gt', cloud, '--samples', '100', '--seed', '4', '--iid'])
    assert (a.samples, a.seed, a.iid) == (100, 4, True)
    assert np.array_equal(es._cloud(cloud, a), pts.astype(np.float64))             # --samples with a vertex-only PLY: its points, as they are
    a = es.parse(['--pr', mesh_path, '--gt', cloud])
    assert a.samples is None and np.array_equal(es._cloud(mesh_path, a), v.astype(np.float64))      # without --samples: the vertices, as before
    for bad in (['--pr', cloud, '--gt', cloud, '--samples', '0'], ['--mesh', mesh_path, '--views', cloud, '--gt-points', cloud, '--samples', '5']):
        with pytest.raises(SystemExit) as ex:
            es.parse(bad)
        assert ex.value.code == 2
    sm = _script('sample_mesh')
    with pytest.raises(SystemExit, match='no faces'):
        sm.main(['--mesh', cloud, '--n', '10', '--out', str(tmp_path / 'out.ply')])
    assert not os.path.exists(tmp_path / 'out.ply')
    with pytest.raises(SystemExit, match='does not exist'):
        sm.main(['--mesh', str(tmp_path / 'missing.ply'), '--out', str(tmp_path / 'out.ply')])
