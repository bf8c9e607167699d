"""CPU tier of the relighter (include/nero_hip_relight.h, nero_amd/relight.py; its binding: tests/test_binding_cpu.py): the entry points
refuse bad arguments before any device call, the launch arithmetic holds at its limit under the sanitizers, the orbit equals the
reference's, the stored roughness is squared once, the RGBA writer round-trips, and the restatement (tests/relight_ref.py) has its closed
forms and stays inside the exemption cap on the committed direction sets."""
import math
import os

import numpy as np
import pytest
import torch

from tests import relight_ref as RR
from tests.helpers import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope='module')
def RL():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight
    return relight


def test_entry_points_refuse_bad_arguments_without_a_device(RL):
    from nero_amd import _lib as L
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    assert lib.nero_bvh_export_faces(None, p) == ERR_ARG and lib.nero_bvh_export_faces(p, None) == ERR_ARG
    for k in (0, 1, 2, 4, 5, 6):
        a = [p, p, p, 4, p, p, p, None]
        a[k] = None
        assert lib.nero_bvh_trace_faces(*a) == ERR_ARG and 'nero_bvh_trace_faces' in err()
    assert lib.nero_bvh_trace_faces(p, p, p, -1, p, p, p, None) == ERR_ARG
    assert lib.nero_bvh_trace_faces(p, p, p, (2 ** 31 - 1) // 3 + 1, p, p, p, None) == ERR_ARG and 'chunks' in err()
    assert lib.nero_bvh_trace_faces(p, p, p, 0, p, p, p, None) == 0
    # nero_env_lookup(env, h, w, convention, rot, dirs, n, clamp_max, rgb, stream)
    for k in (0, 5, 8):
        a = [p, 4, 8, 0, None, p, 4, 0.0, p, None]
        a[k] = None
        assert lib.nero_env_lookup(*a) == ERR_ARG and 'nero_env_lookup' in err()
    for h, w in ((0, 8), (4, 0), (-1, 8), (4, 16385)):
        assert lib.nero_env_lookup(p, h, w, 0, None, p, 4, 0.0, p, None) == ERR_ARG and 'sizes' in err()
    for conv in (-1, 3):
        assert lib.nero_env_lookup(p, 4, 8, conv, None, p, 4, 0.0, p, None) == ERR_ARG and 'convention' in err()
    assert lib.nero_env_lookup(p, 4, 8, 0, None, p, -1, 0.0, p, None) == ERR_ARG
    assert lib.nero_env_lookup(p, 4, 8, 0, None, p, 2 ** 31, 0.0, p, None) == ERR_ARG
    assert lib.nero_env_lookup(p, 4, 8, 2, None, p, 0, 0.0, p, None) == 0
    # nero_relight_rays(pt, tab_d, tab_s, P, Dd, Ds, geometry_type, rays_o, rays_d, dead, stream)
    for k in (0, 1, 2, 7, 8):
        a = [p, p, p, 4, 8, 8, 0, p, p, p, None]
        a[k] = None
        assert lib.nero_relight_rays(*a) == ERR_ARG and 'nero_relight_rays' in err()
    rel = lambda P_, Dd, Ds, g=0, **kw: lib.nero_bvh_relight(*[kw.get(k, v) for k, v in (
        ('handle', p), ('pt', p), ('tab_d', p), ('tab_s', p), ('P', P_), ('Dd', Dd), ('Ds', Ds), ('g', g), ('env', p), ('eh', 4), ('ew', 8),
        ('conv', 2), ('rot', None), ('clamp', 0.0), ('rgb', p), ('dif', None), ('spec', None), ('ws', p), ('wsb', 1 << 40), ('stream', None))])
    for k in ('handle', 'pt', 'tab_d', 'tab_s', 'env', 'rgb'):
        assert rel(4, 8, 8, **{k: None}) == ERR_ARG and 'nero_bvh_relight' in err()
    for Dd, Ds in ((0, 8), (8, 0), (4097, 8), (8, 4097), (-1, 8)):
        assert lib.nero_relight_rays(p, p, p, 4, Dd, Ds, 0, p, p, p, None) == ERR_ARG and '[1, 4096]' in err()
        assert rel(4, Dd, Ds) == ERR_ARG and '[1, 4096]' in err()
        assert lib.nero_relight_workspace_bytes(4, Dd, Ds) == 0
    for P_, Dd, Ds in (((2 ** 31 - 64) // 64 + 1, 1, 1), (1 << 21, 512, 512), (2 ** 31 - 1, 4096, 4096), ((2 ** 31 - 64) // 128 + 1, 60, 5)):
        assert P_ * RL.padded_samples(Dd, Ds) > RL.MAX_LANES
        assert lib.nero_relight_rays(p, p, p, P_, Dd, Ds, 0, p, p, p, None) == ERR_ARG and '2^31 - 64' in err()
        assert rel(P_, Dd, Ds) == ERR_ARG and '2^31 - 64' in err()
        assert lib.nero_relight_workspace_bytes(P_, Dd, Ds) == 0
    assert rel(-1, 8, 8) == ERR_ARG and rel(4, 8, 8, g=2) == ERR_ARG and rel(4, 8, 8, conv=3) == ERR_ARG and 'convention' in err()
    assert rel(4, 8, 8, eh=0) == ERR_ARG and rel(4, 8, 8, ew=0) == ERR_ARG and 'sizes' in err()
    assert rel(4, 8, 8, ws=None) == ERR_ARG and rel(4, 8, 8, wsb=4 * 6 * 4 - 1) == ERR_ARG and 'workspace' in err()
    assert rel(4, 8, 8, ws=4098) == ERR_ARG
    assert lib.nero_relight_workspace_bytes(4, 8, 8) == 4 * 6 * 4 and lib.nero_relight_workspace_bytes(3, 60, 5) == 3 * 2 * 6 * 4
    # nothing to do: no device needed
    assert lib.nero_relight_rays(p, p, p, 0, 8, 8, 0, p, p, None, None) == 0
    assert rel(0, 8, 8, ws=None, wsb=0) == 0 and lib.nero_relight_workspace_bytes(0, 8, 8) == 0


def test_grid_arithmetic_at_the_limit_under_the_sanitizer(tmp_path):
    """nero_amd/csrc/relight_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program): at P * padded(D) = the
    largest admitted total the grid covers every lane, no index passes 2^31 - 1, the workspace holds the last partial and nothing overflows on
    the way"""
    rows = [tuple(int(x) for x in ln.split()) for ln in run_host_program(tmp_path, 'relight_plan_main.cpp').splitlines()]
    assert len(rows) == 18
    for Dd, Ds, P_, total, threads, blocks in rows:
        pad = -(-(Dd + Ds) // 64) * 64
        assert total == P_ * pad and total <= 2 ** 31 - 64 < total + pad
        assert blocks == -(-total // threads) and blocks * threads - 1 <= 2 ** 31 - 1
    assert (1, 1, (2 ** 31 - 64) // 64, 2 ** 31 - 64, 256, 1 << 23) in rows        # total + 255 does not fit an int here


def test_the_orbit_is_the_reference_s(RL):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'relight_poses.npz'))
    assert len(z['args']) == 2
    for i, (num, az, el, dist) in enumerate(z['args']):
        want = z[f'poses{i}']
        got = RL.relighting_poses(int(num), az, el, dist)
        assert got.shape == want.shape == (int(num), 3, 4)
        assert np.abs(got - want).max() < 1e-6
        assert np.abs(RR.relighting_poses(int(num), az, el, dist).numpy() - want).max() < 1e-6
        for pose in got:
            Rm, t = pose[:, :3], pose[:, 3]
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-9 and np.linalg.det(Rm) > 0
            centre = -Rm.T @ t
            assert abs(np.linalg.norm(centre) - dist) < 1e-9
            assert np.abs(Rm[2] - (-centre / dist)).max() < 1e-9                   # the optical axis points at the origin
    K = RL.default_K(600, 800)
    assert K[0, 0] == K[1, 1] == np.float32(800 * 50 / 36) and K[0, 2] == 400 and K[1, 2] == 300


def test_the_sample_table_is_uniform_in_elevation(RL):
    for n in (1, 5, 512):
        tab = RL.sample_table(n)
        assert tab.dtype == torch.float32 and tab.shape == (n, 2) and torch.equal(tab, RR.sample_table(n))
        assert float(tab.min()) >= 0 and float(tab.max()) < 1
        assert torch.equal(torch.floor(tab[:, 1].double() * n).long(), torch.arange(n))          # one sample per stratum


def test_roughness_is_squared_once(RL, tmp_path):
    rng = np.random.default_rng(3)
    stored = {'metallic': rng.uniform(size=(7, 1)).astype(np.float32), 'roughness': rng.uniform(0.1, 1, size=(7, 1)).astype(np.float32),
              'albedo': rng.uniform(size=(7, 3)).astype(np.float32)}
    for k, v in stored.items():
        np.save(tmp_path / f'{k}.npy', v)
    mats = RL.load_materials(str(tmp_path))
    assert sorted(mats) == ['albedo', 'metallic', 'roughness']
    for k in stored:                                                                 # as stored: perceptual
        assert np.array_equal(mats[k], stored[k])
    mat5 = torch.from_numpy(np.concatenate([mats['metallic'], mats['roughness'], mats['albedo']], -1))
    est = RL.estimator_materials(mat5)
    assert torch.equal(est[:, 1], mat5[:, 1] * mat5[:, 1])
    assert torch.equal(est[:, [0, 2, 3, 4]], mat5[:, [0, 2, 3, 4]])


def test_the_rgba_writer_round_trips(RL, tmp_path):
    from nero_amd.texture import png_bytes, read_png
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (5, 7), (32, 32)):
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        path = str(tmp_path / f'{h}x{w}.png')
        RL.write_rgba_png(path, torch.from_numpy(img))
        back = read_png(path)
        assert back.dtype == np.uint8 and np.array_equal(back, img)
    with pytest.raises(ValueError):
        RL.rgba_png_bytes(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        png_bytes(np.zeros((4, 4, 4), np.uint8))                                     # the RGB writer is as it was


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('is_real', [0, 1])
@pytest.mark.parametrize('hw', [(4, 8), (5, 7), (64, 128)])
def test_the_grid_lookup_inverts_the_grid(is_real, hw):
    h, w = hw
    env = RR.proper_map(h, w)
    d = RR.grid_directions(h, w, is_real).reshape(-1, 3)
    got, dec = RR.env_lookup(env, d, is_real)
    assert float((got - env.double().reshape(-1, 3)).abs().max()) < 1e-9
    got32, _ = RR.env_lookup(env, d.float(), is_real)
    assert float((got32 - env.reshape(-1, 3)).abs().max()) < 2e-4 * (w + h) / 12
    assert not bool(RR.exempt(dec).any())


def test_the_equirectangular_lookup_hits_the_stated_texels():
    h, w = 4, 8
    env = torch.arange(h * w * 3, dtype=torch.float64).reshape(h, w, 3)
    # u = atan2(y, -x) / 2 pi + 0.5: -x -> 0.5, +y -> 0.75, +x -> 1 (= 0), -y -> 0.25; texel coordinate u w - 0.5 between two columns
    mid = lambda r, a, b: (env[r, a] + env[r, b]) / 2
    eq = (env[1] + env[2]) / 2                                                       # v = 0.5: between rows 1 and 2
    want = {(-1, 0, 0): (eq[3] + eq[4]) / 2, (0, 1, 0): (eq[5] + eq[6]) / 2, (1, 0, 0): (eq[7] + eq[0]) / 2, (0, -1, 0): (eq[1] + eq[2]) / 2}
    for d, val in want.items():
        got, _ = RR.env_lookup(env, torch.tensor([d], dtype=torch.float64), 2)
        assert float((got[0] - val).abs().max()) < 1e-9, d
    # the poles: row 0 at the top (+z), rows are clamped; atan2(0, -0) = pi puts the pole at u = 1, between the last and the first column
    up, _ = RR.env_lookup(env, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64), 2)
    dn, _ = RR.env_lookup(env, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64), 2)
    assert float((up[0] - mid(0, 7, 0)).abs().max()) < 1e-9 and float((dn[0] - mid(3, 7, 0)).abs().max()) < 1e-9
    # a texel centre reproduces the texel
    u, v = (2 + 0.5) / w, 1 - (1 + 0.5) / h
    az, el = (u - 0.5) * 2 * math.pi, (v - 0.5) * math.pi
    d = torch.tensor([[-math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)]], dtype=torch.float64)
    got, _ = RR.env_lookup(env, d, 2)
    assert float((got[0] - env[1, 2]).abs().max()) < 1e-9
    # rotation first, cap last
    rot = np.asarray([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])                           # +x -> +y
    got, _ = RR.env_lookup(env, torch.tensor([[1.0, 0, 0]], dtype=torch.float64), 2, rot=rot, clamp=50.0)
    assert float((got[0] - torch.clamp(want[(0, 1, 0)], max=50.0)).abs().max()) < 1e-9


@pytest.mark.parametrize('conv', [0, 1, 2])
def test_the_lookup_sets_stay_inside_the_exemption_cap(conv):
    d = RR.lookup_directions()
    for h, w in ((4, 8), (5, 7), (64, 128)):
        env = RR.proper_map(h, w, hot=(h // 2, w // 2, 1000.0))
        for rot in (None, RR.ROT):
            L64, dec = RR.env_lookup(env, d.double(), conv, rot)
            ex = RR.exempt(dec)
            assert float(ex.float().mean()) <= RR.CAP
            L32, _ = RR.env_lookup(env, d, conv, rot)
            rel = ((L32.double() - L64).abs() / torch.clamp(L64.abs(), min=float(env.mean())))[~ex]
            assert float(rel.max()) < 1e-2                                           # float32 against float64: the floor the GPU tier scales


def _diffuse_case(Dd, Ds, seed=0):
    from tests import mc_shade_ref as R
    g = torch.Generator().manual_seed(seed)
    P_ = 16
    n = torch.nn.functional.normalize(torch.randn(P_, 3, generator=g, dtype=torch.float64), dim=-1)
    view = torch.nn.functional.normalize(n + 0.5 * torch.randn(P_, 3, generator=g, dtype=torch.float64), dim=-1)
    mat5 = torch.cat([torch.zeros(P_, 1, dtype=torch.float64), 0.2 + 0.6 * torch.rand(P_, 1, generator=g, dtype=torch.float64),
                      torch.rand(P_, 3, generator=g, dtype=torch.float64)], -1)
    tab_d, tab_s = R._tab(Dd).double(), R._tab(Ds).double()
    pt, _ = R.point_setup(n * 0.5, view, n, mat5, torch.rand(P_, generator=g, dtype=torch.float64), torch.rand(P_, generator=g, dtype=torch.float64))
    w, o = R.dirs(pt, tab_d, tab_s)
    return pt, w, o, mat5


def test_a_constant_map_gives_albedo_times_radiance():
    Dd, Ds = 64, 32
    pt, w, _, mat5 = _diffuse_case(Dd, Ds)
    env = torch.full((4, 8, 3), 1.0, dtype=torch.float64) * torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    free = torch.zeros(w.shape[0], dtype=torch.bool)
    for conv in (0, 1, 2):
        for geom in (0, 1):
            rgb, dif, spec, _ = RR.relight(pt, w, free, free, env, conv, None, 0.0, Dd, Ds, geom)
            assert float((dif - mat5[:, 2:5] * env[0, 0]).abs().max()) < 1e-12
            assert float((rgb - dif - spec).abs().max()) < 1e-12 and float(spec.min()) >= 0
    # everything blocked, or everything dead: black
    for blocked, dead in ((~free, free), (free, ~free)):
        rgb, _, _, _ = RR.relight(pt, w, blocked, dead, env, 2, None, 0.0, Dd, Ds, 0)
        assert float(rgb.abs().max()) == 0.0


def test_the_disk_closed_form_at_the_sample_count_used():
    """a point on a plane with a disk of radius R at height h above it: the cosine-weighted fraction of the hemisphere the disk covers is
    R^2 / (R^2 + h^2), so the diffuse term under a constant map is albedo L0 (1 - R^2 / (R^2 + h^2)).  The 512-direction table the GPU tier
    uses (uniform in sin^2 theta: the relighter's own, not the training table) estimates it within 1.5 %."""
    from tests import mc_shade_ref as R
    Dd, Ds = 512, 16
    Rd, hgt = 0.3, 0.25
    ang = torch.linspace(0, 2 * math.pi, 257, dtype=torch.float64)[:-1]
    V = torch.cat([torch.tensor([[0.0, 0.0, hgt]], dtype=torch.float64), torch.stack([Rd * torch.cos(ang), Rd * torch.sin(ang), torch.full_like(ang, hgt)], -1)])
    Fc = torch.stack([torch.zeros(256, dtype=torch.long), 1 + torch.arange(256), 1 + (torch.arange(256) + 1) % 256], -1)
    n = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)
    mat5 = torch.tensor([[0.0, 0.5, 0.8, 0.6, 0.4]], dtype=torch.float64)
    pt, _ = R.point_setup(torch.zeros(1, 3, dtype=torch.float64), torch.tensor([[0.3, 0.1, 1.0]], dtype=torch.float64), n, mat5,
                          torch.tensor([0.37], dtype=torch.float64), torch.tensor([0.11], dtype=torch.float64))
    w, o = R.dirs(pt, RR.sample_table(Dd).double(), RR.sample_table(Ds).double())
    blocked, dec = RR.occluded(V, Fc, o, w)
    dead, _ = R.dead_rays(pt, w, Dd, Ds, 0)
    env = torch.full((4, 8, 3), 2.0, dtype=torch.float64)
    _, dif, _, _ = RR.relight(pt, w, blocked, dead, env, 2, None, 0.0, Dd, Ds, 0)
    # the polygon's area is that of a disk of radius R sqrt(sin(2 pi / 256) / (2 pi / 256)): 1e-4 below R
    want = mat5[0, 2:5] * 2.0 * (1 - Rd ** 2 / (Rd ** 2 + hgt ** 2))
    assert float(((dif[0] - want) / want).abs().max()) < 0.015
    assert float(RR.exempt(dec).float().mean()) <= RR.CAP


def test_the_brute_force_hit_rebuilds_its_point():
    V, Fc = RR.scene()
    o, d = RR.camera_rays(RR.relighting_poses(3, 20.0, 35.0, 2.0)[1], np.asarray([[60.0, 0, 16], [0, 60.0, 16], [0, 0, 1]]), 32, 32)
    depth, face, bary, _ = RR.closest_hit(V.double(), Fc, o, d)
    hit = face >= 0
    assert 100 < int(hit.sum()) < 1024 and bool((depth[~hit] == RR.MISS_DEPTH).all())
    p = RR.interpolate(V.double(), Fc, face[hit], bary[hit])
    assert float((p - (o[hit] + depth[hit, None] * d[hit])).abs().max()) < 1e-12
    assert float(bary[hit].min()) >= 0 and float(bary[hit].sum(-1).max()) <= 1
