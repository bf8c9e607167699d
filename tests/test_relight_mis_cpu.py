"""CPU tier of the relighter's third strategy (include/nero_hip_envsample.h, nero_amd/csrc/envsample.hip; its binding:
tests/test_binding_cpu.py): the entry points refuse bad arguments before any device call, the launch arithmetic holds at its limits
under the sanitizers, and the restatement (tests/envsample_ref.py) is checked against quadrature: the MIS estimator and the two-strategy
estimator share one expectation (which is what fixes S), and MIS has the smaller error under a map with a hot texel."""
import math

import numpy as np
import pytest
import torch

from tests import envsample_ref as ER
from tests import mc_shade_ref as R
from tests import relight_ref as RR
from tests.helpers import run_host_program

ERR_ARG = -1
F64 = torch.float64


@pytest.fixture(scope='module')
def RL():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight
    return relight


# ---- arguments, plan --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device(RL):
    from nero_amd import _lib as L
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    # nero_env_cdf(env, eh, ew, convention, rot, clamp_max, ws, cdf, info, weights, stream)
    cdf = lambda **kw: lib.nero_env_cdf(*[kw.get(k, v) for k, v in (('env', p), ('eh', 4), ('ew', 8), ('conv', 2), ('rot', None), ('clamp', 0.0),
                                                                    ('ws', 4096), ('cdf', p), ('info', p), ('weights', None), ('stream', None))])
    for k in ('env', 'ws', 'cdf', 'info'):
        assert cdf(**{k: None}) == ERR_ARG and 'nero_env_cdf' in err()
    assert cdf(eh=0) == ERR_ARG and cdf(ew=16385) == ERR_ARG and 'sizes' in err()
    assert cdf(conv=3) == ERR_ARG and 'convention' in err()
    assert cdf(eh=8192, ew=8193) == ERR_ARG and '2^26' in err() and cdf(eh=16384, ew=16384) == ERR_ARG and '2^26' in err()
    assert cdf(ws=4096 + 8) == ERR_ARG and 'aligned' in err()
    assert lib.nero_env_cdf_workspace_bytes(0, 8) == 0 and lib.nero_env_cdf_workspace_bytes(8192, 8193) == 0 and '2^26' in err()
    # nero_relight_mis_rays(pt, tab_d, tab_s, tab_l, rand_l, P, Dd, Ds, Dl, geometry_type, cdf, info, gh, gw, rays_o, rays_d, dead, cell, pdf_l, stream)
    rays = lambda P_=4, Dd=8, Ds=8, Dl=8, g=0, **kw: lib.nero_relight_mis_rays(*[kw.get(k, v) for k, v in (
        ('pt', p), ('tab_d', p), ('tab_s', p), ('tab_l', p), ('rand_l', None), ('P', P_), ('Dd', Dd), ('Ds', Ds), ('Dl', Dl), ('g', g), ('cdf', p),
        ('info', p), ('gh', 4), ('gw', 8), ('ro', p), ('rd', p), ('dead', None), ('cell', None), ('pdf', None), ('stream', None))])
    # nero_bvh_relight_mis(handle, pt, tab_d, tab_s, tab_l, rand_l, P, Dd, Ds, Dl, g, env, eh, ew, conv, rot, clamp, cdf, info, rgb, dif, spec, ws, wsb, stream)
    rel = lambda P_=4, Dd=8, Ds=8, Dl=8, g=0, **kw: lib.nero_bvh_relight_mis(*[kw.get(k, v) for k, v in (
        ('handle', p), ('pt', p), ('tab_d', p), ('tab_s', p), ('tab_l', p), ('rand_l', None), ('P', P_), ('Dd', Dd), ('Ds', Ds), ('Dl', Dl), ('g', g),
        ('env', p), ('eh', 4), ('ew', 8), ('conv', 2), ('rot', None), ('clamp', 0.0), ('cdf', p), ('info', p), ('rgb', p), ('dif', None),
        ('spec', None), ('ws', p), ('wsb', 1 << 40), ('stream', None))])
    for k in ('pt', 'tab_d', 'tab_s', 'tab_l', 'cdf', 'info', 'ro', 'rd'):
        assert rays(**{k: None}) == ERR_ARG and 'nero_relight_mis_rays' in err()
    for k in ('handle', 'pt', 'tab_d', 'tab_s', 'tab_l', 'cdf', 'info', 'rgb', 'env'):
        assert rel(**{k: None}) == ERR_ARG and 'nero_bvh_relight_mis' in err()
    for Dd, Ds, Dl in ((8, 8, 0), (8, 8, 4097), (8, 8, -1), (0, 8, 8), (8, 4097, 8)):
        assert rays(Dd=Dd, Ds=Ds, Dl=Dl) == ERR_ARG and '[1, 4096]' in err()
        assert rel(Dd=Dd, Ds=Ds, Dl=Dl) == ERR_ARG and '[1, 4096]' in err()
        assert lib.nero_relight_mis_workspace_bytes(4, Dd, Ds, Dl) == 0
    for P_, Dd, Ds, Dl in (((2 ** 31 - 64) // 64 + 1, 1, 1, 1), (1 << 21, 512, 256, 256), (2 ** 31 - 1, 4096, 4096, 4096),
                           ((2 ** 31 - 64) // 128 + 1, 60, 4, 1)):
        assert P_ * RL.padded_samples(Dd, Ds, Dl) > RL.MAX_LANES
        assert rays(P_, Dd, Ds, Dl) == ERR_ARG and '2^31 - 64' in err()
        assert rel(P_, Dd, Ds, Dl) == ERR_ARG and '2^31 - 64' in err()
        assert lib.nero_relight_mis_workspace_bytes(P_, Dd, Ds, Dl) == 0
    assert rays(g=2) == ERR_ARG and rel(g=-1) == ERR_ARG and 'geometry_type' in err()
    assert rays(P_=-1) == ERR_ARG and rel(P_=-1) == ERR_ARG
    assert rays(gh=0) == ERR_ARG and rays(gh=8192, gw=8193) == ERR_ARG and '2^26' in err()
    assert rel(eh=0) == ERR_ARG and 'sizes' in err() and rel(conv=3) == ERR_ARG and rel(eh=8192, ew=8193) == ERR_ARG and '2^26' in err()
    assert rel(ws=None) == ERR_ARG and rel(wsb=4 * 6 * 4 - 1) == ERR_ARG and 'workspace' in err() and rel(ws=4098) == ERR_ARG
    assert lib.nero_relight_mis_workspace_bytes(4, 8, 8, 8) == 4 * 6 * 4 and lib.nero_relight_mis_workspace_bytes(3, 60, 4, 1) == 3 * 2 * 6 * 4
    # nothing to do: no device needed
    assert rays(P_=0) == 0 and rel(P_=0, ws=None, wsb=0) == 0 and lib.nero_relight_mis_workspace_bytes(0, 8, 8, 8) == 0


def test_plan_arithmetic_at_the_limits_under_the_sanitizer(tmp_path):
    """nero_amd/csrc/envsample_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program)"""
    stdout = run_host_program(tmp_path, 'envsample_plan_main.cpp')
    maps = [tuple(int(x) for x in ln.split()[1:]) for ln in stdout.splitlines() if ln.startswith('map')]
    mis = [tuple(int(x) for x in ln.split()[1:]) for ln in stdout.splitlines() if ln.startswith('mis')]
    assert len(maps) == 9 and len(mis) == 16
    for eh, ew, N, B, fixed in maps:
        assert N == eh * ew and B == ER.weight_bits(N) == min(40, 62 - (N - 1).bit_length()) and (N << B) <= 2 ** 62
        assert fixed == 256 + -(-N * 4 // 256) * 256 + -(-N * 8 // 256) * 256
    for Dd, Ds, Dl, P_, total, threads, blocks in mis:
        pad = -(-(Dd + Ds + Dl) // 64) * 64
        assert total == P_ * pad and total <= 2 ** 31 - 64 < total + pad
        assert blocks == -(-total // threads) and blocks * threads - 1 <= 2 ** 31 - 1
    assert (1, 1, 1, (2 ** 31 - 64) // 64, 2 ** 31 - 64, 256, 1 << 23) in mis


def test_pixel_shifts_chain_after_the_rotations(RL):
    idx = torch.arange(1000, dtype=torch.int64)
    s = RL.pixel_shifts(idx, 7)
    assert s.shape == (1000, 2) and s.dtype == torch.float32 and float(s.min()) >= 0 and float(s.max()) < 1
    m = 0xffffffff
    h2 = (RL.pixel_rotations(idx, 7)[1].double() * 2 ** 24).long()                  # the top 24 bits of h2 only: redo the chain from h1
    h1 = RL._lowbias32((idx * 0x9E3779B9 + 7) & m)
    h2_full = RL._lowbias32((h1 + 0x68E31DA4) & m)
    assert torch.equal(h2_full >> 8, h2)
    h3 = RL._lowbias32((h2_full + 0x68E31DA4) & m)
    h4 = RL._lowbias32((h3 + 0x68E31DA4) & m)
    assert torch.equal(s[:, 0], (h3 >> 8).float() * 2.0 ** -24) and torch.equal(s[:, 1], (h4 >> 8).float() * 2.0 ** -24)
    assert abs(float(s.mean()) - 0.5) < 0.03 and not torch.equal(RL.pixel_shifts(idx, 8), s)


# ---- the inversion --------------------------------------------------------------------------------------------------------------------------
def _table(env, conv=2, rot=None, clamp=0.0):
    a, fb = ER.weights(env, conv, rot, clamp, torch.float32)
    return ER.table_from_weights(a.numpy(), fb)


def test_inversion_edge_cases():
    gh, gw = 16, 32
    env = RR.proper_map(gh, gw, hot=(5, 9, 1000.0))
    env[8:13] = 0.0                                         # rows 8 .. 12 are black: the bilinear lookup at a centre of rows 9 .. 11 reads
    cdf, info = _table(env)                                 # black rows only, whichever side its float32 row coordinate falls
    Rm = cdf.reshape(gh, gw)[:, -1]
    assert info[0] == cdf[-1] > 0 and info[4] == 0 and Rm[11] == Rm[10] == Rm[9] == Rm[8] and info[1] >= 3 * gw
    lo, hi = np.float32(0.0), np.float32(1 - 2.0 ** -24)
    u = np.asarray([lo, hi, lo, hi, 0.5], np.float32)
    v = np.asarray([lo, lo, hi, hi, 0.25], np.float32)
    row, col, x1, x2, wc = ER.draw(cdf, gh, gw, u, v)
    assert row[0] == 0 and col[0] == 0 and x1[0] == 0 and x2[0] == 0                # u = 0: the first cell, its corner
    assert row[1] == gh - 1 and col[3] == gw - 1 and (wc > 0).all()
    assert (x1 >= 0).all() and (x1 <= 1 - 2.0 ** -24).all() and (x2 >= 0).all() and (x2 <= 1 - 2.0 ** -24).all()
    # a dense lattice: zero-weight rows and cells are never chosen, every cell's share of the samples follows its weight
    g = torch.Generator().manual_seed(3)
    uu = torch.rand(200000, 2, generator=g).numpy().astype(np.float32)
    row, col, x1, x2, wc = ER.draw(cdf, gh, gw, uu[:, 0], uu[:, 1])
    assert (wc > 0).all() and not np.isin(row, (9, 10, 11)).any()
    w = np.diff(np.concatenate([[0], cdf]))
    assert np.array_equal(wc, w[row * gw + col])
    share = np.bincount(row * gw + col, minlength=gh * gw) / len(row)
    assert np.abs(share - w / w.sum()).max() < 4 * math.sqrt(0.25 / len(row))
    # the residuals are uniform inside the cell: the lattice stays stratified
    assert abs(x1.mean() - 0.5) < 0.01 and abs(x2.mean() - 0.5) < 0.01
    # one non-zero cell: every sample falls inside it
    one = torch.zeros(6, 10, 3)
    a = np.zeros(60, np.float32)
    a[3 * 10 + 7] = 2.5
    cdf1, info1 = ER.table_from_weights(a)
    assert info1[1] == 59 and info1[2] == 2 and info1[3] == 40 and info1[0] == int(2.5 * 2 ** 38)
    row, col, x1, x2, wc = ER.draw(cdf1, 6, 10, uu[:5000, 0], uu[:5000, 1])
    assert (row == 3).all() and (col == 7).all() and (wc == info1[0]).all()
    assert np.abs(x1 - uu[:5000, 0]).max() < 1e-6 and np.abs(x2 - uu[:5000, 1]).max() < 1e-6      # the cell IS the unit square here
    # a black map takes the fallback: uniform in solid angle, p_l = 1 / (4 pi) to rounding away from the poles
    a, fb = ER.weights(one, 2, None, 0.0, torch.float32)
    assert fb and float(a.min()) > 0
    cdfb, infob = ER.table_from_weights(a.numpy(), fb)
    assert infob[4] == 1 and infob[2] == 0 and infob[1] == 0
    gh, gw = 64, 128
    a, fb = ER.weights(torch.zeros(gh, gw, 3), 2, None, 0.0, torch.float32)
    cdfb, infob = ER.table_from_weights(a.numpy(), fb)
    row, col, x1, x2, wc = ER.draw(cdfb, gh, gw, uu[:20000, 0], uu[:20000, 1])
    vc = 1.0 - (torch.from_numpy(row).double() + 0.5) / gh                            # at the cell's own centre the density is exact
    pdf = ER.pdf_light(cdfb, gh, gw, row * gw + col, vc)
    # the sum of cos el over the rows is gh / (pi/2 ...) only up to the midpoint rule: 1 + O(1 / gh^2)
    assert float((pdf * 4 * math.pi - 1).abs().max()) < 2.0 / gh ** 2 + 1e-6
    mid = (row > 4) & (row < gh - 5)
    v = 1.0 - (torch.from_numpy(row).double() + torch.from_numpy(x1)) / gh
    pdf = ER.pdf_light(cdfb, gh, gw, row * gw + col, v)
    assert float((pdf * 4 * math.pi - 1).abs()[torch.from_numpy(mid)].max()) < 0.5 * math.pi / gh * math.tan(math.pi / 2 * (1 - 10.0 / gh)) + 1e-3


def test_the_density_integrates_to_one():
    """p_l over the sphere by midpoint quadrature in (u, v), for a hot-texel map under a rotation and for the fallback"""
    for env, rot in ((RR.proper_map(16, 32, hot=(5, 9, 1000.0)), RR.ROT), (torch.zeros(5, 7, 3), None)):
        gh, gw = env.shape[:2]
        cdf, info = _table(env, 1 if rot is not None else 2, rot)
        n = 8
        r, c, i, j = torch.meshgrid(torch.arange(gh), torch.arange(gw), torch.arange(n), torch.arange(n), indexing='ij')
        v = (1.0 - (r.double() + (i.double() + 0.5) / n) / gh).reshape(-1)
        cell = (r * gw + c).reshape(-1).numpy()
        pdf = ER.pdf_light(cdf, gh, gw, cell, v)
        dw = torch.cos((v - 0.5) * math.pi) * (2 * math.pi * math.pi) / (gh * gw * n * n)
        assert abs(float((pdf * dw).sum()) - 1.0) < 1e-9


# ---- quadrature: one expectation, less noise --------------------------------------------------------------------------------------------------
SEEDS = range(16)
ALPHAS, METALLICS = (0.09, 0.36, 0.81), (0.0, 1.0)


def _quadrature_points(RL, seed, metallic=None):
    """the six points (alpha x metallic) at one place, a tilted view, with the lattice shifts of `seed` -> pt [6,32] float64, rand_l [6,2]"""
    n = torch.nn.functional.normalize(torch.tensor([[0.1, -0.5, 0.85]], dtype=F64), dim=-1).expand(6, 3)
    t = torch.nn.functional.normalize(torch.linalg.cross(n, torch.tensor([[0.0, 0.0, 1.0]], dtype=F64).expand(6, 3)), dim=-1)
    view = 0.6 * n + 0.8 * t
    mat5 = torch.tensor([[m if metallic is None else metallic, a, 0.8, 0.5, 0.3] for a in ALPHAS for m in METALLICS], dtype=F64)
    idx = torch.arange(6, dtype=torch.int64)
    rd, rs = RL.pixel_rotations(idx, seed)
    pt, _ = R.point_setup(torch.zeros(6, 3, dtype=F64), view, n, mat5, rd.double(), rs.double())
    return pt, RL.pixel_shifts(idx, seed)


@pytest.fixture(scope='module')
def quadrature(RL):
    env = RR.proper_map(16, 32, hot=(5, 9, 1000.0))
    cdf, info = _table(env)
    free = lambda n: torch.zeros(n, dtype=torch.bool)
    out = {}
    for name, metallic in (('as_is', None), ('metallic_0', 0.0)):
        mis, two = [], []
        for seed in SEEDS:
            pt, rand_l = _quadrature_points(RL, seed, metallic)
            Dd, Ds, Dl = 64, 64, 128
            tabs = [RR.sample_table(k).double() for k in (Dd, Ds, Dl)]
            w, o, dead, cell, pdf, _, _ = ER.mis_rays(pt, tabs[0], tabs[1], tabs[2], rand_l, cdf, 16, 32, 0)
            mis.append(torch.stack(ER.relight_mis(pt, w, free(len(w)), dead, pdf, env, 2, None, 0.0, Dd, Ds, Dl, 0)))
            Dd, Ds = 128, 128
            tabs = [RR.sample_table(k).double() for k in (Dd, Ds)]
            w, o = R.dirs(pt, tabs[0], tabs[1])
            dead, _ = R.dead_rays(pt, w, Dd, Ds, 0)
            two.append(torch.stack(RR.relight(pt, w, free(len(w)), dead, env, 2, None, 0.0, Dd, Ds, 0)[:3]))
        out[name] = (torch.stack(mis), torch.stack(two))                            # [seed, (rgb, diffuse, spec), point, channel]
    pt, _ = _quadrature_points(RL, 0)
    se = torch.stack([x.std(0, unbiased=True) / 4 for x in out['as_is']])
    se_min = float(se[se > 0].min())
    n, prev = 256, None
    while True:
        I = ER.integrals(pt, env, 2, 0, n)
        if prev is not None and max(float((a - b).abs().max()) for a, b in zip(I, prev)) < 0.1 * se_min:
            break
        prev, n = I, 2 * n
        assert n <= 4096, 'the quadrature did not settle'
    I0 = (I[0][0:1].expand(6, 3), None, None)           # the metallic-0 copies: one normal, one albedo -- the diffuse integral of point 0
    return out, I, I0, n


def test_both_estimators_have_the_expectation_of_the_integrals(quadrature):
    """(a) the mean over 16 lattice shifts of the MIS restatement at (64, 64, 128) and (b) of the two-strategy restatement at (128, 128) are
    within 4 standard errors (the shifts' own sample deviation / 4) of I_diff + I_cos + I_ggx, the two-strategy estimator's expectation
    term by term (envsample_ref.integrals).  I_cos + I_ggx is the issue's "2 I_spec"; the quadrature puts it at 2.03 I_cos for alpha = 0.09
    and at 1.5 .. 1.7 I_cos for alpha = 0.36 and 0.81 (the GGX samples are divided by a density they do not have), which is why S is a
    function of the direction and not the constant 2.  Measured: every |mean - expectation| below 2.2 standard errors for both estimators,
    at relative standard errors of 0.2 .. 0.4 % (MIS) and 0.4 .. 1.4 % (two-strategy)."""
    out, (I_diff, I_cos, I_ggx), _, n = quadrature
    want = I_diff + I_cos + I_ggx
    print(f'S = (I_cos + I_ggx) / I_cos per point:\n{(I_cos + I_ggx) / I_cos}')
    for name, est in zip(('MIS (64, 64, 128)', 'two-strategy (128, 128)'), out['as_is']):
        mean, se = est[:, 0].mean(0), est[:, 0].std(0, unbiased=True) / 4
        z = (mean - want).abs() / se
        print(f'{name}: quadrature grid {n} x {2 * n}; |mean - (I_diff + 2 I_spec)| / standard error per point (rows: alpha x metallic):\n{z}\n'
              f'relative standard error:\n{se / want}')
        assert bool((z <= 4).all()), name


def test_mis_has_the_smaller_error_at_equal_sample_count(quadrature):
    """(c) at equal D = 256 the RMS error over the shifts is smaller for MIS: the diffuse term at every point (on the metallic-0 copy of the
    points, where it is not identically zero), rgb at the metallic-0 points.  Measured MIS / two-strategy: diffuse 0.16 .. 0.31, rgb
    0.03 .. 0.25."""
    out, (I_diff, I_cos, I_ggx), (I0_diff, _, _), _ = quadrature
    rms = lambda est, want: torch.sqrt(((est - want[None]) ** 2).mean(0)).max(-1)[0]
    d_mis, d_two = rms(out['metallic_0'][0][:, 1], I0_diff), rms(out['metallic_0'][1][:, 1], I0_diff)
    want = I_diff + I_cos + I_ggx
    r_mis, r_two = rms(out['as_is'][0][:, 0], want), rms(out['as_is'][1][:, 0], want)
    print(f'RMS error over 16 shifts, MIS / two-strategy: diffuse {(d_mis / d_two).tolist()}, rgb {(r_mis / r_two).tolist()}')
    assert bool((d_mis < d_two).all())
    m0 = torch.tensor([m == 0.0 for _ in ALPHAS for m in METALLICS])
    assert bool((r_mis[m0] < r_two[m0]).all())


# ---- the committed inputs of the GPU tier -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Dd,Ds,Dl', ER.MIS_CASES)
def test_the_sample_set_cases_stay_inside_the_exemption_cap(Dd, Ds, Dl):
    """the looked-up cell of a direction of the two BRDF strategies is a discontinuous decision: the GPU tier exempts a ray whose float64
    direction lies within MARGIN of a cell border (or of the grid's axis), and at most CAP of the rays of a case may be"""
    P_ = 65
    c, tab_d, tab_s, tab_l = ER.candidates(P_, Dd, Ds, Dl)
    pt, _ = R.point_setup(c['pts'].double(), c['view'].double(), c['normals'].double(), c['mat5'].double(), c['rand_d'].double(), c['rand_s'].double())
    env, conv, rot, clamp = ER.env_of_case(Dd + Dl)
    cdf, _ = _table(env, conv, rot, clamp or 0.0)
    for geom, rand_l in ((0, c['rand_l']), (1, None)):
        w, o, dead, cell, pdf, margin, is_light = ER.mis_rays(pt, tab_d, tab_s, tab_l, rand_l, cdf, 16, 32, geom)
        ex = margin < RR.MARGIN
        assert float(ex.double().mean()) <= RR.CAP and not bool(ex[is_light].any())
        assert bool(torch.isfinite(pdf).all()) and float(pdf.min()) >= 0 and cell.min() >= 0 and cell.max() < 512
        if geom == 1:
            assert not bool(dead.any())


def test_the_restatement_under_a_constant_map():
    """the pixels of the GPU tier's convex-mesh test, rebuilt here by brute force: under a constant map, metallic 0, the float64 restatement's
    diffuse term at 64 + 64 + 64 samples is within 0.021 of albedo L0 (measured: 2.03e-2 at the worst of 510 pixels); the GPU tier allows
    twice that for its own, slightly different, points"""
    from nero_amd import relight as RL
    V, Fc = RR.scene(quad=False)
    pose = RR.relighting_poses(4, 30.0, 60.0, 2.4)[1].numpy()
    Km = np.asarray([[60.0, 0, 24], [0, 60.0, 24], [0, 0, 1]], np.float32)
    o, d = RR.camera_rays(pose, Km, 48, 48)
    depth, face, bary, _ = RR.closest_hit(V.double(), Fc, o, d)
    idx = torch.nonzero(face >= 0)[:, 0]
    corner = V.double()[Fc[face[idx]]]
    n = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    n = torch.where((n * d[idx]).sum(-1, keepdim=True) > 0, -n, n)
    g = torch.Generator().manual_seed(1)
    m = len(idx)
    alb = torch.tensor([0.8, 0.5, 0.25], dtype=F64)
    mat5 = torch.cat([torch.zeros(m, 1, dtype=F64), (0.2 + 0.7 * torch.rand(m, 1, generator=g, dtype=F64)) ** 2, alb.expand(m, 3)], -1)
    rd, rs = RL.pixel_rotations(idx, 0)
    pt, _ = R.point_setup(RR.interpolate(V.double(), Fc, face[idx], bary[idx]), -d[idx], n, mat5, rd.double(), rs.double())
    L0 = torch.tensor([0.5, 1.0, 3.0])
    env = L0.expand(4, 8, 3).contiguous()
    cdf, info = _table(env, 0)
    tab = RR.sample_table(64).double()
    w, _, dead, cell, pdf, _, _ = ER.mis_rays(pt, tab, tab, tab, RL.pixel_shifts(idx, 0), cdf, 4, 8, 0)
    dif = ER.relight_mis(pt, w, torch.zeros(len(w), dtype=torch.bool), dead, pdf, env, 0, None, 0.0, 64, 64, 64, 0)[1]
    rel = float(((dif - alb * L0.double()) / (alb * L0.double())).abs().max())
    print(f'constant map, {m} pixels: restatement / (albedo L0) - 1 = {rel:.2e}')
    assert m > 100 and rel <= 0.021
