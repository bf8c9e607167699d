"""CPU tier of the relighter's one bounce (include/nero_hip_bounce.h, nero_amd/csrc/relight_estimator.hip; its binding:
tests/test_binding_cpu.py): the entry points refuse bad arguments before any device call, the workspace arithmetic holds at its limits
under the sanitizers, and the restatement (tests/bounce_ref.py) is checked against closed forms and quadrature: a point under a disk, the
one-sample secondary estimator's expectation, a convex mesh.  The committed cases of the GPU tier are checked here, with the restatement
alone, for the share of lanes that bounce and for the share of points a decision margin exempts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import bounce_ref as B
from tests import envsample_ref as ER
from tests import mc_shade_ref as R
from tests import relight_ref as RR
from tests.helpers import run_host_program

ERR_ARG = -1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def RL():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight
    return relight


# ---- 1. binding: tests/test_binding_cpu.py.  2. arguments -----------------------------------------------------------------------------------
class _Bvh(C.Structure):
    _fields_ = [('d_nodes', C.c_void_p), ('d_tris', C.c_void_p), ('d_face', C.c_void_p), ('n_nodes', C.c_int), ('n_tris', C.c_int)]


class _Handle(C.Structure):                # nero_bvh::Handle (bvh_types.h), made on the host: the calls below are refused before it is followed
    _fields_ = [('b', _Bvh), ('root', C.c_int), ('max_depth', C.c_int), ('mode', C.c_int)]


def test_entry_points_refuse_bad_arguments_without_a_device(RL):
    from nero_amd import _lib as L
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed
    hd = _Handle(_Bvh(p, p, p, 11, 12), 0, 4, 0)                      # a tree of 12 triangles
    h = C.addressof(hd)
    err = lambda: lib.nero_last_error().decode()
    mesh = (('verts', p), ('V', 9), ('tris', p), ('T', 12), ('mat5', p), ('normals', None), ('key', None))
    two = lambda P_=4, Dd=8, Ds=8, g=0, **kw: lib.nero_bvh_relight_bounce(*[kw.get(k, v) for k, v in (
        ('handle', h), ('pt', p), ('tab_d', p), ('tab_s', p), ('P', P_), ('Dd', Dd), ('Ds', Ds), ('g', g), ('env', p), ('eh', 4), ('ew', 8), ('conv', 2),
        ('rot', None), ('clamp', 0.0)) + mesh + (('rgb', p), ('dif', None), ('spec', None), ('ind', None), ('ws', p), ('wsb', 1 << 40), ('stream', None))])
    mis = lambda P_=4, Dd=8, Ds=8, Dl=8, g=0, **kw: lib.nero_bvh_relight_mis_bounce(*[kw.get(k, v) for k, v in (
        ('handle', h), ('pt', p), ('tab_d', p), ('tab_s', p), ('tab_l', p), ('rand_l', None), ('P', P_), ('Dd', Dd), ('Ds', Ds), ('Dl', Dl), ('g', g),
        ('env', p), ('eh', 4), ('ew', 8), ('conv', 2), ('rot', None), ('clamp', 0.0), ('cdf', p), ('info', p)) + mesh + (
        ('rgb', p), ('dif', None), ('spec', None), ('ind', None), ('ws', p), ('wsb', 1 << 40), ('stream', None))])
    rays = lambda P_=4, Dd=8, Ds=8, Dl=8, g=0, **kw: lib.nero_relight_bounce_rays(*[kw.get(k, v) for k, v in (
        ('handle', h), ('pt', p), ('tab_d', p), ('tab_s', p), ('tab_l', p), ('rand_l', None), ('P', P_), ('Dd', Dd), ('Ds', Ds), ('Dl', Dl), ('g', g),
        ('cdf', p), ('info', p), ('gh', 4), ('gw', 8)) + mesh + (('state', None), ('face', None), ('bary', None), ('sec_o', None), ('sec_d', None),
                                                               ('strategy', None), ('pdf_l', None), ('cell', None), ('stream', None))])
    # null pointers
    for k in ('handle', 'pt', 'tab_d', 'tab_s', 'rgb', 'env', 'verts', 'tris', 'mat5'):
        assert two(**{k: None}) == ERR_ARG and 'nero_bvh_relight_bounce' in err(), k
    for k in ('handle', 'pt', 'tab_d', 'tab_s', 'tab_l', 'cdf', 'info', 'rgb', 'env', 'verts', 'tris', 'mat5'):
        assert mis(**{k: None}) == ERR_ARG and 'nero_bvh_relight_mis_bounce' in err(), k
    for k in ('handle', 'pt', 'tab_d', 'tab_s', 'cdf', 'info', 'verts', 'tris', 'mat5'):
        assert rays(**{k: None}) == ERR_ARG and 'nero_relight_bounce_rays' in err(), k
    assert rays(tab_l=None, Dl=8) == ERR_ARG and 'Dl must be 0' in err()
    # the mesh is not the tree's
    for call in (two, mis, rays):
        assert call(T=11) == ERR_ARG and 'T = 11' in err() and '12 triangles' in err()
        assert call(V=0) == ERR_ARG and 'V must be' in err()
    # sample limits
    for Dd, Ds in ((0, 8), (8, 0), (4097, 8), (8, 4097)):
        assert two(Dd=Dd, Ds=Ds) == ERR_ARG and '[1, 4096]' in err()
        assert rays(Dd=Dd, Ds=Ds, Dl=0, tab_l=None) == ERR_ARG and '[1, 4096]' in err()
        assert lib.nero_relight_bounce_workspace_bytes(4, Dd, Ds) == 0
    for Dd, Ds, Dl in ((8, 8, 0), (8, 8, 4097), (8, 8, -1), (0, 8, 8), (8, 4097, 8)):
        assert mis(Dd=Dd, Ds=Ds, Dl=Dl) == ERR_ARG and '[1, 4096]' in err()
        assert rays(Dd=Dd, Ds=Ds, Dl=Dl) == ERR_ARG and '[1, 4096]' in err()
        assert lib.nero_relight_mis_bounce_workspace_bytes(4, Dd, Ds, Dl) == 0
    for P_, Dd, Ds, Dl in (((2 ** 31 - 64) // 64 + 1, 1, 1, 1), (1 << 22, 512, 256, 256), (2 ** 31 - 1, 4096, 4096, 4096)):
        assert P_ * RL.padded_samples(Dd, Ds, Dl) > RL.MAX_LANES and P_ * RL.padded_samples(Dd, Ds) > RL.MAX_LANES
        assert mis(P_, Dd, Ds, Dl) == ERR_ARG and '2^31 - 64' in err() and rays(P_, Dd, Ds, Dl) == ERR_ARG and '2^31 - 64' in err()
        assert two(P_, Dd, Ds) == ERR_ARG and '2^31 - 64' in err()
        assert lib.nero_relight_mis_bounce_workspace_bytes(P_, Dd, Ds, Dl) == 0 and lib.nero_relight_bounce_workspace_bytes(P_, Dd, Ds) == 0
    assert two(g=2) == ERR_ARG and mis(g=-1) == ERR_ARG and rays(g=2) == ERR_ARG and 'geometry_type' in err()
    assert two(P_=-1) == ERR_ARG and mis(P_=-1) == ERR_ARG and rays(P_=-1) == ERR_ARG
    assert two(eh=0) == ERR_ARG and 'sizes' in err() and mis(conv=3) == ERR_ARG and 'convention' in err()
    assert mis(eh=8192, ew=8193) == ERR_ARG and '2^26' in err() and rays(gh=0) == ERR_ARG and '2^26' in err()
    # the workspace: twelve floats per wavefront
    assert two(ws=None) == ERR_ARG and 'workspace' in err() and two(wsb=4 * 12 * 4 - 1) == ERR_ARG and 'nero_relight_bounce_workspace_bytes' in err()
    assert two(ws=4098) == ERR_ARG and 'misaligned' in err()
    assert mis(ws=None) == ERR_ARG and mis(wsb=4 * 12 * 4 - 1) == ERR_ARG and 'nero_relight_mis_bounce_workspace_bytes' in err() and mis(ws=4097) == ERR_ARG
    assert lib.nero_relight_bounce_workspace_bytes(4, 8, 8) == 4 * 12 * 4 and lib.nero_relight_bounce_workspace_bytes(3, 60, 5) == 3 * 2 * 12 * 4
    assert lib.nero_relight_mis_bounce_workspace_bytes(4, 8, 8, 8) == 4 * 12 * 4 and lib.nero_relight_mis_bounce_workspace_bytes(3, 60, 4, 1) == 3 * 2 * 12 * 4
    # nothing to do: no device needed
    assert two(P_=0, ws=None, wsb=0) == 0 and mis(P_=0, ws=None, wsb=0) == 0 and rays(P_=0) == 0
    assert lib.nero_relight_bounce_workspace_bytes(0, 8, 8) == 0
    # the Python layer
    with pytest.raises(ValueError, match='bounces'):
        RL.relight_points(None, torch.zeros(1, 32), torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(2, 4, 3), bounces=2)
    with pytest.raises(ValueError, match='mesh'):
        RL.relight_points(None, torch.zeros(1, 32), torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(2, 4, 3), bounces=1)


# ---- 3. the workspace arithmetic ------------------------------------------------------------------------------------------------------------
def test_workspace_arithmetic_at_the_limits_under_the_sanitizers(tmp_path):
    """nero_amd/csrc/relight_plan.h with the bounce's partial, as a stand-alone program under the sanitizers (tests.helpers.run_host_program)"""
    stdout = run_host_program(tmp_path, 'relight_bounce_plan_main.cpp')
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in stdout.splitlines() if ln.startswith('bounce')]
    assert len(rows) == 22
    for Dd, Ds, Dl, P_, total, nbytes, threads, blocks in rows:
        pad = -(-(Dd + Ds + Dl) // 64) * 64
        assert total == P_ * pad and total <= 2 ** 31 - 64 < total + pad
        assert nbytes == total // 64 * 12 * 4 and blocks == -(-total // threads) and blocks * threads - 1 <= 2 ** 31 - 1
    assert (1, 1, 0, (2 ** 31 - 64) // 64, 2 ** 31 - 64, (2 ** 31 - 64) // 64 * 48, 256, 1 << 23) in rows


# ---- the hash -------------------------------------------------------------------------------------------------------------------------------
def test_pixel_keys_chain_after_the_shifts_and_the_variates_are_uniform(RL):
    idx = torch.arange(1000, dtype=torch.int64)
    m = 0xffffffff
    h = RL._lowbias32((idx * 0x9E3779B9 + 7) & m)
    for _ in range(3):
        h = RL._lowbias32((h + 0x68E31DA4) & m)
    assert torch.equal(RL.pixel_shifts(idx, 7)[:, 1], (h >> 8).float() * 2.0 ** -24)                 # h4, the last hash of pixel_shifts
    key = RL.pixel_keys(idx, 7)
    assert key.dtype == torch.int64 and torch.equal(key, RL._lowbias32((h + 0x68E31DA4) & m)) and int(key.min()) >= 0 and int(key.max()) < 2 ** 32
    assert not torch.equal(RL.pixel_keys(idx, 8), key)
    assert torch.equal(torch.from_numpy(B.lowbias32(np.arange(1000, dtype=np.uint64)).astype(np.int64)), RL._lowbias32(idx))
    u1, u2, u3 = B.variates(key.numpy(), 256)
    for u in (u1, u2, u3):
        assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1 and abs(float(u.mean()) - 0.5) < 4 * math.sqrt(1 / 12 / u.size)
    assert abs(np.corrcoef(u1.reshape(-1), u2.reshape(-1))[0, 1]) < 0.01 and abs(np.corrcoef(u2.reshape(-1), u3.reshape(-1))[0, 1]) < 0.01
    k2 = B.variates(key.numpy()[::-1].copy(), 256)[0]                                               # (pixel, j) alone: not the position in the chunk
    assert np.array_equal(k2[::-1], u1)
    s, margin = B.strategy(u1, 16, 16, 32)
    assert abs((s == 0).mean() - 0.25) < 0.01 and abs((s == 2).mean() - 0.5) < 0.01 and margin.min() >= 0
    s2, _ = B.strategy(u1, 3, 2, 0)
    assert set(np.unique(s2)) == {0, 1} and abs((s2 == 0).mean() - 0.6) < 0.01                       # never the table without one


# ---- the restatement's own parts --------------------------------------------------------------------------------------------------------------
def _records(n, seed=0, dtype=F64):
    g = torch.Generator().manual_seed(600 + seed)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=-1)
    view = torch.nn.functional.normalize(nrm + 0.8 * torch.randn(n, 3, generator=g, dtype=F64), dim=-1)
    mat5 = torch.cat([torch.rand(n, 1, generator=g, dtype=F64), 0.09 + 0.8 * torch.rand(n, 1, generator=g, dtype=F64),
                      0.1 + 0.8 * torch.rand(n, 3, generator=g, dtype=F64)], -1)
    return R.point_setup(torch.randn(n, 3, generator=g, dtype=F64), view, nrm, mat5, None, None)[0].to(dtype)


def test_the_per_row_directions_and_the_per_sample_term_are_those_of_the_references_they_stand_on():
    n = 40
    rec = _records(n)
    g = torch.Generator().manual_seed(5)
    tab = torch.rand(n, 2, generator=g, dtype=F64)
    want_d = R.diffuse_dirs(rec, tab)[torch.arange(n), torch.arange(n)]                              # row i with table row i
    want_s = R.specular_dirs(rec, tab)[torch.arange(n), torch.arange(n)]
    assert torch.equal(B.cosine_dir(rec, tab[:, 0], tab[:, 1]), want_d) and torch.equal(B.ggx_dir(rec, tab[:, 0], tab[:, 1]), want_s)
    # L_o of one sample = D x the mean envsample_ref.mis_estimator takes over a one-sample set
    w2 = torch.nn.functional.normalize(rec[:, 3:6] + 0.7 * torch.randn(n, 3, generator=g, dtype=F64), dim=-1)
    Le, pl = torch.rand(n, 3, generator=g, dtype=F64), torch.rand(n, generator=g, dtype=F64)
    for Dd, Ds, Dl, geom in ((16, 16, 32, 0), (33, 32, 7, 1), (3, 2, 0, 0)):
        Lo, Lo_d, Lo_s = B.radiance(rec, w2, pl, Le, Dd, Ds, Dl, geom)
        rgb, dif, spec = ER.mis_estimator(rec, w2[:, None], Le[:, None], pl[:, None], Dd, Ds, Dl, geom)
        D = Dd + Ds + Dl
        assert torch.allclose(Lo, rgb * D, rtol=1e-13, atol=0) and torch.allclose(Lo_d, dif * D, rtol=1e-13, atol=0)
        assert torch.allclose(Lo_s, spec * D, rtol=1e-13, atol=0) and float(Lo.min()) >= 0
        capped = B.radiance(rec, w2, pl, Le, Dd, Ds, Dl, geom, clamp=0.5)[0]
        assert torch.equal(capped, torch.clamp(Lo, max=0.5))


# ---- 4. closed form: a point under a disk -----------------------------------------------------------------------------------------------------
def test_a_point_under_a_disk_direct_and_indirect():
    """A point at the origin, normal +z, under a disk of radius R at height h (form factor F = R^2 / (R^2 + h^2)) with albedo rho, metallic 0,
    roughness 1, in a uniform map of radiance 1; a tiny upward triangle lies at the origin.  Direct diffuse: albedo (1 - F).  Indirect,
    through the secondary's diffuse term and the primary's diffuse term: albedo rho F -- every point of the disk sees the whole lower
    hemisphere free (the triangle subtends 1e-5 sr).  The bound on the indirect term is 3 x the lattice's own error on the direct term at
    the same sample count.  Sample count (512, 1): the lattice error is that of Dd = 512 cosine samples on the disk's rim; the indirect
    term meets the same rim through the same lanes and adds the noise of one hashed sample per lane, which is small only where the mixture
    is close to the cosine density: the diffuse per-sample term is (NoL / pi) / p_mix2 = D / (Dd + Ds p_act / p_d), constant up to Ds / Dd.
    With Ds = 1 that is 0.2 % per lane; with Ds = 16 it is 3 % per lane and the hashed noise alone (measured: 1.2e-3 absolute) is 4.6 x the
    lattice's error (2.6e-4) -- the estimator is right there too, but the bound is not a statement about it."""
    Dd, Ds, Rd, hgt = 512, 1, 0.3, 0.25
    rho, alb = torch.tensor([0.7, 0.5, 0.3], dtype=F64), torch.tensor([0.8, 0.6, 0.4], dtype=F64)
    ang = torch.linspace(0, 2 * math.pi, 257, dtype=F64)[:-1]
    V = torch.cat([torch.tensor([[0.0, 0.0, hgt]], dtype=F64), torch.stack([Rd * torch.cos(ang), Rd * torch.sin(ang), torch.full_like(ang, hgt)], -1),
                   torch.tensor([[-1e-3, -1e-3, 0.0], [1e-3, -1e-3, 0.0], [0.0, 1e-3, 0.0]], dtype=F64)])
    Fc = torch.cat([torch.stack([torch.zeros(256, dtype=torch.long), 1 + (torch.arange(256) + 1) % 256, 1 + torch.arange(256)], -1),   # facing down
                    torch.tensor([[257, 258, 259]])])                                                                                 # facing up
    mat5 = torch.cat([torch.zeros(len(V), 1, dtype=F64), torch.ones(len(V), 1, dtype=F64), rho.expand(len(V), 3)], -1)
    pt, _ = R.point_setup(torch.zeros(1, 3, dtype=F64), torch.tensor([[0.3, 0.1, 1.0]], dtype=F64), torch.tensor([[0.0, 0.0, 1.0]], dtype=F64),
                          torch.cat([torch.tensor([0.0, 0.25], dtype=F64), alb])[None], torch.tensor([0.37], dtype=F64), torch.tensor([0.11], dtype=F64))
    w, o, dead, _ = B.primary_rays(pt, RR.sample_table(Dd, F64), RR.sample_table(Ds, F64), None, None, None, 0)
    mesh, key = (V, Fc, mat5, None), np.asarray([12345])
    state, face, bary, blocked2, _ = B.facts(pt, w, o, dead, None, key, mesh, Dd, Ds, 0, 0)
    out = B.bounce(pt, w, None, state, face, bary, blocked2, key, mesh, torch.ones(4, 8, 3, dtype=F64), 2, None, 0.0, Dd, Ds, 0, 0)
    Ff = Rd ** 2 / (Rd ** 2 + hgt ** 2)
    e_dir = float((out['diffuse'][0] - alb * (1 - Ff)).abs().max())
    e_ind = float((out['indirect_sd'][0][0] - alb * rho * Ff).abs().max())
    print(f'point under a disk, ({Dd}, {Ds}): F = {Ff:.4f}, {float((state == B.BOUNCED).float().mean()):.1%} of the lanes bounce, {int(blocked2.sum())} '
          f'second shadow rays blocked; direct diffuse off albedo (1 - F) by {e_dir:.2e} (the lattice), indirect off albedo rho F by {e_ind:.2e} '
          f'({e_ind / e_dir:.2f} x)')
    assert int((face[state == B.BOUNCED] < 256).all()) and int(blocked2.sum()) == 0 and 0 < e_dir < 1e-3
    assert e_ind <= 3 * e_dir
    assert torch.allclose(out['indirect'], sum(out['indirect_sd']) + sum(out['indirect_ss']), rtol=1e-12, atol=0)
    assert torch.allclose(out['rgb'], out['diffuse'] + out['spec'] + out['indirect'], rtol=1e-14, atol=0)


# ---- 5. the one-sample secondary estimator against quadrature ---------------------------------------------------------------------------------
ALPHAS, METALLICS = (0.09, 0.36, 0.81), (0.0, 1.0)


def test_the_one_sample_secondary_estimator_has_the_expectation_of_the_integrals():
    """At six (normal, view, material) settings -- alpha 0.09, 0.36, 0.81 x metallic 0, 1, three normals and views -- under an unoccluded
    map: the mean of L_o over 2^16 hashed samples (fixed key) against Int (f_d + f S) L dw = I_diff + I_cos + I_ggx of envsample_ref.integrals,
    within 4 of its own standard errors, for the shares of a MIS primary (16, 16, 32) and of a two-strategy primary (3, 2)."""
    N = 1 << 16
    nrm = torch.nn.functional.normalize(torch.tensor([[0.1, -0.5, 0.85], [0.7, 0.2, -0.4], [-0.3, 0.6, 0.5]], dtype=F64), dim=-1)[[0, 1, 2, 0, 1, 2]]
    t = torch.nn.functional.normalize(torch.linalg.cross(nrm, torch.tensor([[0.0, 0.0, 1.0]], dtype=F64).expand(6, 3)), dim=-1)
    view = 0.6 * nrm + 0.8 * t
    mat5 = torch.tensor([[m, a, 0.8, 0.5, 0.3] for a in ALPHAS for m in METALLICS], dtype=F64)
    rec6, _ = R.point_setup(torch.zeros(6, 3, dtype=F64), view, nrm, mat5, None, None)
    env = RR.proper_map(16, 32, seed=3)
    a32, fb = ER.weights(env, 2, None, 0.0, F32)
    cdf, _ = ER.table_from_weights(a32.numpy(), fb)
    means, ses = {}, {}
    for Dd, Ds, Dl in ((16, 16, 32), (3, 2, 0)):
        for k in range(6):
            u1, u2, u3 = B.variates(np.asarray([977 + k]), N)
            s, _ = B.strategy(u1[0], Dd, Ds, Dl)
            rec = rec6[k:k + 1].expand(N, 32)
            w2, _, dead2, pl, _ = B.secondary(rec, s, u2[0], u3[0], (cdf, 16, 32) if Dl else None, 0)
            Le, _ = RR.env_lookup(env, w2, 2)
            Le = torch.where(dead2[:, None], torch.zeros_like(Le), Le)
            Lo = B.radiance(rec, w2, pl, Le, Dd, Ds, Dl, 0)[0]
            means[(Dd, Ds, Dl, k)], ses[(Dd, Ds, Dl, k)] = Lo.mean(0), Lo.std(0, unbiased=True) / math.sqrt(N)
    se_min = min(float(v.min()) for v in ses.values())
    n, prev = 512, None
    while True:
        I = ER.integrals(rec6, env, 2, 0, n)
        if prev is not None and max(float((a - b).abs().max()) for a, b in zip(I, prev)) < 0.1 * se_min:
            break
        prev, n = I, 2 * n
        assert n <= 4096, 'the quadrature did not settle'
    want = I[0] + I[1] + I[2]
    worst = 0.0
    for (Dd, Ds, Dl, k), mean in means.items():
        z = ((mean - want[k]).abs() / ses[(Dd, Ds, Dl, k)])
        worst = max(worst, float(z.max()))
        print(f'shares ({Dd}, {Ds}, {Dl}) alpha {float(mat5[k, 1]):.2f} metallic {float(mat5[k, 0]):.0f}: mean {mean.tolist()} expectation {want[k].tolist()} '
              f'rel. s.e. {float((ses[(Dd, Ds, Dl, k)] / want[k]).max()):.2%}, off by {float(z.max()):.2f} s.e.')
    print(f'quadrature settled at n = {n}; worst {worst:.2f} standard errors')
    assert worst <= 4.0


# ---- 6. a convex mesh -------------------------------------------------------------------------------------------------------------------------
def test_no_indirect_light_on_a_convex_mesh():
    """points just above the plain icosphere with their normals pointing away from it: no lane is blocked (a GGX sample below the horizon is
    dead, geometry type 0) and the indirect term is exactly 0; a few normals tilted into the sphere show the test can tell"""
    V, Fc = RR.scene(3, quad=False)
    P_, Dd, Ds, Dl = 24, 24, 16, 8
    g = torch.Generator().manual_seed(31)
    d = torch.nn.functional.normalize(torch.randn(P_, 3, generator=g, dtype=F64), dim=-1)
    nrm = d.clone()
    nrm[-4:] = torch.nn.functional.normalize(d[-4:] + 2.0 * torch.linalg.cross(d[-4:], torch.tensor([[0.0, 0.0, 1.0]], dtype=F64).expand(4, 3)), dim=-1)
    mat5 = torch.cat([torch.rand(P_, 1, generator=g, dtype=F64), 0.1 + 0.8 * torch.rand(P_, 1, generator=g, dtype=F64),
                      0.1 + 0.8 * torch.rand(P_, 3, generator=g, dtype=F64)], -1)
    pt, _ = R.point_setup(d * 0.503, torch.nn.functional.normalize(nrm + 0.3 * d, dim=-1), nrm, mat5, torch.rand(P_, generator=g, dtype=F64),
                          torch.rand(P_, generator=g, dtype=F64))
    env = RR.proper_map(16, 32, seed=1)
    a32, fb = ER.weights(env, 2, None, 0.0, F32)
    cdf, _ = ER.table_from_weights(a32.numpy(), fb)
    mesh, key = (V, Fc, B.vertex_materials(len(V)).double(), None), np.arange(P_) * 7919
    for dl in (0, Dl):
        tabs = [RR.sample_table(k, F64) for k in (Dd, Ds)] + [RR.sample_table(dl, F64) if dl else None]
        w, o, dead, pdf = B.primary_rays(pt, tabs[0], tabs[1], tabs[2], torch.rand(P_, 2, generator=g), (cdf, 16, 32), 0)
        state, face, bary, blocked2, _ = B.facts(pt, w, o, dead, pdf, key, mesh, Dd, Ds, dl, 0, (cdf, 16, 32))
        out = B.bounce(pt, w, pdf, state, face, bary, blocked2, key, mesh, env, 2, None, 0.0, Dd, Ds, dl, 0, (cdf, 16, 32))
        hits = (state.reshape(P_, -1) >= B.BOUNCED).sum(-1)
        free = hits == 0
        if dl == 0:                                                    # (a light sample may point anywhere: into the sphere too)
            assert bool(free[:-4].all())
        assert int(free.sum()) >= 4 and bool((hits[-4:] > 0).all())
        assert not out['indirect'][free].any() and bool((out['indirect'][-4:].sum(-1) > 0).all()) and float(out['indirect'].min()) >= 0
        assert torch.equal(out['rgb'][free], (out['diffuse'] + out['spec'])[free])


# ---- the committed cases of the GPU tier ------------------------------------------------------------------------------------------------------
def _case_on_the_cpu(i, P_, Dd, Ds, Dl, mesh, geom):
    s = B.case_inputs(i, P_, Dd, Ds, Dl, mesh)
    c = s['c']
    pt, _ = R.point_setup(*[c[k].double() for k in ('pts', 'view', 'normals', 'mat5', 'rand_d', 'rand_s')])
    table = None
    if Dl:
        a32, fb = ER.weights(s['env'], s['conv'], s['rot'], s['clamp'] or 0.0, F32)
        table = (ER.table_from_weights(a32.numpy(), fb)[0], 16, 32)
    w, o, dead, pdf = B.primary_rays(pt, s['tab_d'].double(), s['tab_s'].double(), None if not Dl else s['tab_l'].double(), c['rand_l'], table, geom)
    m = (s['V'], s['Fc'], s['vmat5'], s['normals'])
    state, face, bary, blocked2, dec_f = B.facts(pt, w, o, dead, pdf, s['key'], m, Dd, Ds, Dl, geom, table)
    out = B.bounce(pt, w, pdf, state, face, bary, blocked2, s['key'], m, s['env'], s['conv'], s['rot'], s['clamp'] or 0.0, Dd, Ds, Dl, geom, table)
    return state, out, B.exempt(out['dec'], B.CONTINUOUS_KEYS)


@pytest.mark.parametrize('i,P_,Dd,Ds,Dl,mesh,geom', [c for c in B.cases() if c[5] == 'corner' or c[1] <= 65])
def test_the_committed_gpu_cases_bounce_and_stay_inside_the_exemption_cap(i, P_, Dd, Ds, Dl, mesh, geom):
    """with the restatement alone (float64, brute-force walks): on the corner at least 20 % of the lanes bounce; at most 2 % of a case's
    points lie within relight_ref.MARGIN of a decision the kernel takes in floating point and does not report (a frame tie, the
    flat normal's side; the dead flags, the strategies and the cells are reported: bounce_ref.CONTINUOUS_KEYS).  The sphere's cases of 1000 points are left to the GPU tier, which asserts the same cap with the device's
    walks: their brute force takes minutes here."""
    state, out, ex = _case_on_the_cpu(i, P_, Dd, Ds, Dl, mesh, geom)
    share = float((state >= B.BOUNCED).float().mean())
    print(f'case {i} ({mesh}, P {P_}, ({Dd}, {Ds}, {Dl}), geom {geom}): {share:.1%} of the lanes bounce, {int(ex.sum())} of {P_} points exempt; '
          f'mean indirect / mean rgb = {float(out["indirect"].mean() / out["rgb"].mean()):.3f}')
    if mesh == 'corner' and P_ * (Dd + Ds + Dl) >= 64:
        assert share >= 0.2
    assert float(ex.float().mean()) <= RR.CAP
    assert bool(torch.isfinite(out['rgb']).all()) and float(out['indirect'].min()) >= 0
