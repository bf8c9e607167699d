"""GPU tier of the relighter: the face table of both BVH builders, nero_bvh_trace_faces, nero_env_lookup, nero_relight_rays and the fused
nero_bvh_relight against the torch restatement (tests/relight_ref.py), reproducibility, closed forms, and the Python layer end to end.

Tolerances: for every compared output the bound is K_FLOOR (4) x the distance between the restatement evaluated in float32 and in float64 on
the same inputs, computed here, relative to max(|value|, mean map radiance) and pooled per condition class (mc_shade_ref's regular / extreme
points, fewer than 16 directions apart), so that an extreme row never loosens a regular one.  Every test prints its kernel / floor ratio
before it asserts."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mc_shade_ref as R
from tests import relight_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
K = RR.K_FLOOR
ULP = 2.0 ** -23                      # a float32 floor below one ulp of the value is an accident of the row, not a measure


@pytest.fixture(scope='module')
def RL():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import relight
    return relight


@pytest.fixture(scope='module')
def L(RL):
    from nero_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def mesh():
    return RR.scene()


@pytest.fixture(scope='module')
def tracers(RL, mesh):
    from nero_amd.raytracing import RayTracer
    V, Fc = mesh
    return {'host': RayTracer(V.numpy(), Fc.int().numpy(), build='host'), 'device': RayTracer(V.cuda(), Fc.int().cuda(), build='device')}


def _export(L, tr):
    info = tr.info()
    nodes = np.zeros((max(info['n_nodes'], 1), 16), np.float32)
    tris = np.zeros((info['n_tris'], 12), np.float32)
    L.check(L.lib.nero_bvh_export(tr._handle(), nodes.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p)))
    return tris


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the face table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('build', ['host', 'device'])
def test_the_face_table_names_the_exported_triangles(RL, L, mesh, tracers, build):
    V, Fc = mesh
    V, Fc = V.numpy(), Fc.numpy()
    face = RL.export_faces(tracers[build])
    assert face.dtype == np.int32 and np.array_equal(np.sort(face), np.arange(len(Fc)))
    rec = _export(L, tracers[build])
    v0, v1, v2 = V[Fc[face, 0]], V[Fc[face, 1]], V[Fc[face, 2]]
    assert np.array_equal(rec[:, 0:3].view(np.int32), v0.view(np.int32))
    assert np.array_equal(rec[:, 3:6], v1 - v0) and np.array_equal(rec[:, 6:9], v2 - v0)
    assert not rec[:, 9:12].any()


@pytest.mark.parametrize('nT', [1, 2, 4])
def test_a_root_leaf_tree_through_the_c_abi(RL, L, nT):
    """trees of at most four triangles are one leaf and no node (RayTracer refuses them: the C ABI does not)"""
    V = np.asarray([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-1, -1, 0.5], [1, -1, 0.5], [1, 1, 0.5], [-1, 1, 0.5]], np.float32) * 0.5
    Fc = np.asarray([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)[:nT].copy()
    h = C.c_void_p()
    L.check(L.lib.nero_bvh_create(V.ctypes.data_as(C.c_void_p), len(V), Fc.ctypes.data_as(C.c_void_p), nT, C.byref(h)))
    try:
        face = np.empty(nT, np.int32)
        L.check(L.lib.nero_bvh_export_faces(h, face.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(np.sort(face), np.arange(nT))
        g = torch.Generator().manual_seed(nT)
        o = torch.cat([torch.rand(64, 2, generator=g) * 1.2 - 0.6, torch.full((64, 1), 2.0)], -1).cuda()
        d = torch.tensor([[0.0, 0.0, -1.0]]).expand(64, 3).contiguous().cuda()
        depth = torch.empty(64, device='cuda')
        fid = torch.empty(64, dtype=torch.int32, device='cuda')
        bary = torch.empty(64, 2, device='cuda')
        pos, nrm, dref = (torch.empty(64, 3, device='cuda'), torch.empty(64, 3, device='cuda'), torch.empty(64, device='cuda'))
        L.check(L.lib.nero_bvh_trace_faces(h, o.data_ptr(), d.data_ptr(), 64, depth.data_ptr(), fid.data_ptr(), bary.data_ptr(), L.stream_ptr()))
        L.check(L.lib.nero_bvh_trace(h, o.data_ptr(), d.data_ptr(), 64, pos.data_ptr(), nrm.data_ptr(), dref.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(_bits(depth), _bits(dref))
        want_d, want_f, want_b, _ = RR.closest_hit(torch.from_numpy(V).double(), torch.from_numpy(Fc), o.cpu().double(), d.cpu().double())
        hit = want_f >= 0
        assert torch.equal(fid.cpu() >= 0, hit) and 0 < int(hit.sum()) < 64
        p = RR.interpolate(torch.from_numpy(V).double(), torch.from_numpy(Fc), fid.cpu()[hit], bary.cpu()[hit].double())
        assert float((p - pos.cpu().double()[hit]).abs().max()) < 1e-6
    finally:
        L.lib.nero_bvh_destroy(h)


# ---- 2. trace_faces -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rays(mesh):
    g = torch.Generator().manual_seed(21)
    pose = RR.relighting_poses(5, 40.0, 50.0, 2.2)[2]
    o1, d1 = RR.camera_rays(pose, np.asarray([[110.0, 0, 50], [0, 110.0, 50], [0, 0, 1]]), 100, 100, F32)
    o2 = (torch.rand(10000, 3, generator=g) * 2 - 1) * 1.2
    d2 = torch.nn.functional.normalize(torch.randn(10000, 3, generator=g), dim=-1)
    d2[:3000] = torch.nn.functional.normalize(-o2[:3000] + 0.3 * torch.randn(3000, 3, generator=g), dim=-1)     # towards the mesh
    return torch.cat([o1, o2]).float().contiguous(), torch.cat([d1, d2]).float().contiguous()


@pytest.fixture(scope='module')
def brute(mesh, rays):
    V, Fc = mesh
    o, d = rays
    return {dt: RR.closest_hit(V.to(dt), Fc, o.to(dt), d.to(dt)) for dt in (F32, F64)}


@pytest.mark.parametrize('build', ['host', 'device'])
def test_trace_faces(RL, L, mesh, tracers, rays, brute, build):
    V, Fc = mesh
    tr = tracers[build]
    o, d = rays[0].cuda(), rays[1].cuda()
    out = {}
    for mode in (0, 1):
        L.check(L.lib.nero_bvh_set_traversal(tr._handle(), mode))
        out[mode] = RL.trace_faces(tr, o, d)
        pos, _, depth = tr.trace(o, d)
        assert torch.equal(_bits(out[mode][0]), _bits(depth))
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                  # the two walks: the same bits
    depth, face, bary = (t.cpu() for t in out[1])
    hit = face >= 0
    assert torch.equal(hit, depth < 10.0) and torch.equal(~hit, depth == 10.0) and 3000 < int(hit.sum()) < 17000
    assert int(face.max()) < len(Fc) and bool((face[hit] >= 1280).any())               # some rays meet the occluder
    assert float(bary[hit].min()) >= 0 and float(bary[hit].sum(-1).max()) <= 1 and not bary[~hit].any()
    # the rebuilt point: the float32 floor is the brute-force restatement's own float32 against float64
    d32, f32_, b32, _ = brute[F32]
    d64, f64_, b64, margin = brute[F64]
    both = (f32_ >= 0) & (f64_ >= 0)
    p32 = RR.interpolate(V, Fc, f32_[both], b32[both])
    p64 = RR.interpolate(V.double(), Fc, f64_[both], b64[both])
    floor = float((p32.double() - p64).abs().max())
    got = RR.interpolate(V.double(), Fc, face[hit], bary[hit].double())
    e_trace = float((got - pos.cpu().double()[hit]).abs().max())
    ex = margin < RR.MARGIN
    assert float(ex.float().mean()) <= RR.CAP
    keep = ~ex
    assert torch.equal(hit[keep], f64_[keep] >= 0)
    sel = keep & hit
    got_all = torch.zeros(len(face), 3, dtype=F64)
    got_all[hit] = got
    want_all = torch.zeros(len(face), 3, dtype=F64)
    want_all[f64_ >= 0] = RR.interpolate(V.double(), Fc, f64_[f64_ >= 0], b64[f64_ >= 0])
    e_brute = float((got_all[sel] - want_all[sel]).abs().max())
    print(f'trace_faces[{build}]: float32 floor {floor:.2e}; rebuilt point vs trace position {e_trace:.2e} ({e_trace / floor:.2f} floors), '
          f'vs brute force {e_brute:.2e} ({e_brute / floor:.2f} floors); {int(ex.sum())} of {len(ex)} rays exempt')
    assert e_trace <= K * floor and e_brute <= K * floor


# ---- 3. the environment lookup --------------------------------------------------------------------------------------------------------------
def _lookup_case(RL, env, d, conv, rot, clamp):
    got = RL.env_lookup(env.cuda(), d.cuda(), conv, rot, clamp).cpu()
    L64, dec = RR.env_lookup(env, d.double(), conv, rot, clamp or 0.0)
    L32, _ = RR.env_lookup(env, d, conv, rot, clamp or 0.0)
    ex = RR.exempt(dec)
    assert float(ex.float().mean()) <= RR.CAP
    floor, err = RR.floors_and_errors(got, L32, L64, float(env.mean()))
    return float(floor[~ex].max()), float(err[~ex].max())


@pytest.mark.parametrize('conv', [0, 1, 2])
def test_env_lookup(RL, conv):
    d = RR.lookup_directions()
    g = torch.Generator().manual_seed(9)
    for h, w in ((4, 8), (5, 7), (64, 128)):
        maps = [RR.proper_map(h, w, hot=(h // 2, w // 2, 1000.0))]
        if conv == 2:
            maps.append(0.2 + torch.rand(h, w, 3, generator=g))                      # any map is a function of the direction here
        for env in maps:
            for rot in (None, RR.ROT):
                for clamp in (None, 1.0):
                    floor, err = _lookup_case(RL, env, d, conv, rot, clamp)
                    print(f'env_lookup conv {conv} {h}x{w} rot {rot is not None} clamp {clamp}: floor {floor:.2e} kernel {err:.2e} '
                          f'({err / max(floor, ULP):.2f} floors)')
                    assert err <= K * max(floor, ULP)


@pytest.mark.parametrize('is_real', [0, 1])
def test_env_lookup_inverts_latlong_directions(RL, is_real):
    from nero_amd.envlight import latlong_directions
    for h, w in ((4, 8), (5, 7), (64, 128)):
        env = RR.proper_map(h, w, seed=3)
        d = latlong_directions(h, w, is_real).reshape(-1, 3)
        got = RL.env_lookup(env.cuda(), d, is_real).cpu()
        L64, _ = RR.env_lookup(env, d.cpu().double(), is_real)
        L32, _ = RR.env_lookup(env, d.cpu(), is_real)
        floor, err = RR.floors_and_errors(got, L32, L64, float(env.mean()))
        floor, err = max(float(floor.max()), ULP), float(err.max())
        back = float((got - env.reshape(-1, 3)).abs().max() / env.mean())
        print(f'round trip is_real {is_real} {h}x{w}: floor {floor:.2e} kernel {err:.2e} ({err / floor:.2f} floors), map reproduced to {back:.2e}')
        assert err <= K * floor and back <= (K + 1) * floor


# ---- points for the sample set and the fused kernel ------------------------------------------------------------------------------------------
DD_DS = ((1, 1), (5, 3), (64, 64), (96, 160), (512, 256))
PS = (1, 63, 65, 1000)


def _points(RL, P_, Dd, Ds):
    """mc_shade_ref's candidates (every fourth point an extreme one: roughness 0.04^2 and 1, NoV = 0, back-facing view, axis-aligned or
    zero normal), moved outside the sphere so that part of their rays is blocked -> pt [P,32] on the GPU (nero_mc_point_setup), class [P]"""
    tab_d, tab_s = RR.sample_table(Dd), RR.sample_table(Ds)
    g = torch.Generator().manual_seed(500 + 7 * P_ + 13 * Dd + Ds)
    c = R._point_candidates(P_, g, tab_d, tab_s)
    pts = torch.nn.functional.normalize(c['pts'], dim=-1) * (0.52 + 0.3 * torch.rand(P_, 1, generator=g))
    pt = RL.point_records(pts.cuda(), c['view'].cuda(), c['normals'].cuda(), c['mat5'].cuda(), c['rand_d'].cuda(), c['rand_s'].cuda())
    return pt, tab_d.cuda(), tab_s.cuda(), c['cls']


# ---- 4. the sample set ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Dd,Ds', DD_DS)
def test_relight_rays_are_the_rays_of_mc_dirs(RL, L, Dd, Ds):
    P_ = 65
    pt, tab_d, tab_s, _ = _points(RL, P_, Dd, Ds)
    D = Dd + Ds
    for geom in (0, 1):
        ro, rd, dead = RL.relight_rays(pt, tab_d, tab_s, geom)
        dirs, orig = torch.empty(P_ * D, 3, device='cuda'), torch.empty(P_ * D, 3, device='cuda')
        dead_mc = torch.empty(P_ * D, dtype=torch.uint8, device='cuda')
        L.check(L.lib.nero_mc_dirs(pt.data_ptr(), tab_d.data_ptr(), tab_s.data_ptr(), P_, Dd, Ds, dirs.data_ptr(), orig.data_ptr(), L.stream_ptr()))
        L.check(L.lib.nero_mc_dead_rays(pt.data_ptr(), dirs.data_ptr(), P_, Dd, Ds, geom, dead_mc.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        p = pt.cpu()
        w32, o32 = R.dirs(p, tab_d.cpu(), tab_s.cpu())
        w64, o64 = R.dirs(p.double(), tab_d.cpu().double(), tab_s.cpu().double())
        floor = max(float((w32.double() - w64).abs().max()), float((o32.double() - o64).abs().max()), ULP)
        e_mc = max(float((rd - dirs).abs().max()), float((ro - orig).abs().max()))
        e_ref = max(float((rd.cpu().double() - w64).abs().max()), float((ro.cpu().double() - o64).abs().max()))
        _, dec = R.dead_rays(p.double(), w64, Dd, Ds, geom)
        close = torch.zeros(P_, D, dtype=torch.bool)
        close[:, Dd:] = dec['dead_margin'][1] < RR.MARGIN
        differ = (dead != dead_mc).cpu().reshape(P_, D)
        print(f'relight_rays ({Dd},{Ds}) geom {geom}: floor {floor:.2e}; vs nero_mc_dirs {e_mc:.2e} ({e_mc / floor:.2f} floors), vs float64 '
              f'{e_ref:.2e} ({e_ref / floor:.2f} floors); dead flags differ on {int(differ.sum())} rays, {int(close.sum())} within the margin')
        # (the distance from float64 is printed, not asserted: at the roughness floor sin(theta) = sqrt(1 - cos^2 + 1e-6) cancels, one rounding
        #  of cos^2 moves the direction by 3e-5, and whether a float32 evaluation meets that rounding is luck -- the two kernels meet the same)
        assert e_mc <= K * floor
        assert not bool((differ & ~close).any())
        if geom == 1:
            assert not bool(dead.any())
        else:
            assert not bool(dead.reshape(P_, D)[:, :Dd].any())


# ---- 5. fused = composed --------------------------------------------------------------------------------------------------------------------
def _env_of_case(i):
    """(map, convention, rotation, cap): the conventions in turn, every other case rotated, every third capped"""
    conv = i % 3
    env = RR.proper_map(16, 32, seed=i, hot=(5, 9, 1000.0))
    return env, conv, (RR.ROT if i % 2 else None), (50.0 if i % 3 == 1 else None)


@pytest.fixture(scope='module')
def fused(RL, tracers):
    """every case once: the kernel's own rays (nero_relight_rays), nero_bvh_occluded on them, the restatement in float32 and float64 from
    those -> {(Dd, Ds, P, geom): (floor [P], err [P], class key [P])} for rgb, diffuse and specular together"""
    tr = tracers['device']
    out = {}
    for i, (Dd, Ds) in enumerate(DD_DS):
        for P_ in PS:
            pt, tab_d, tab_s, cls = _points(RL, P_, Dd, Ds)
            env, conv, rot, clamp = _env_of_case(i + P_)
            for geom in (0, 1):
                got = RL.relight_points(tr, pt, tab_d, tab_s, env.cuda(), conv, rot, clamp, geom)
                ro, rd, dead = RL.relight_rays(pt, tab_d, tab_s, geom)
                blocked = tr.occluded(ro, rd, skip=dead).bool().cpu()
                dead, w, p = dead.bool().cpu(), rd.cpu(), pt.cpu()
                r32 = RR.relight(p, w, blocked, dead, env, conv, rot, clamp or 0.0, Dd, Ds, geom)
                r64 = RR.relight(p.double(), w.double(), blocked, dead, env, conv, rot, clamp or 0.0, Dd, Ds, geom)
                scale = float(env.mean())
                fe = [RR.floors_and_errors(got[k].cpu(), r32[k], r64[k], scale) for k in range(3)]
                floor = torch.stack([f for f, _ in fe]).max(0)[0]
                err = torch.stack([e for _, e in fe]).max(0)[0]
                key = [(geom, int(c), Dd + Ds < 16) for c in cls]
                lit = float((~(blocked | dead)).float().mean())
                out[(Dd, Ds, P_, geom)] = (floor, err, key, lit, bool(torch.isfinite(got[0]).all()))
    pooled = {}
    for floor, _, key, _, _ in out.values():
        for f, k in zip(floor.tolist(), key):
            pooled[k] = max(pooled.get(k, ULP), f)
    return out, pooled


@pytest.mark.parametrize('geom', [0, 1])
@pytest.mark.parametrize('P_', PS)
@pytest.mark.parametrize('Dd,Ds', DD_DS)
def test_fused_equals_composed(fused, Dd, Ds, P_, geom):
    out, pooled = fused
    floor, err, key, lit, finite = out[(Dd, Ds, P_, geom)]
    assert finite
    ratio = {}
    for e, k in zip(err.tolist(), key):
        ratio[k] = max(ratio.get(k, 0.0), e / pooled[k])
    print(f'fused ({Dd},{Ds}) P {P_} geom {geom}: {lit:.0%} of the rays lit; kernel / pooled float32 floor per (geom, class, D < 16): '
          + ', '.join(f'{k}: {v:.2f} (floor {pooled[k]:.1e})' for k, v in sorted(ratio.items())))
    assert max(ratio.values()) <= K


# ---- 6. reproducibility ---------------------------------------------------------------------------------------------------------------------
def _materials(nV, seed=0):
    g = np.random.default_rng(seed)
    return {'metallic': g.uniform(0, 1, (nV, 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (nV, 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (nV, 3)).astype(np.float32)}


@pytest.fixture(scope='module')
def relighter(RL, mesh, tracers):
    V, Fc = mesh
    env = RR.proper_map(16, 32, seed=2, hot=(3, 20, 100.0))
    return RL.Relighter(V, Fc, _materials(len(V)), env, convention='blender', tracer=tracers['device'])


POSE = RR.relighting_poses(4, 30.0, 60.0, 2.4)[1].numpy()
KMAT = np.asarray([[60.0, 0, 24], [0, 60.0, 24], [0, 0, 1]], np.float32)


def test_the_same_bits_on_every_run_and_for_every_chunk(RL, tracers, relighter):
    pt, tab_d, tab_s, _ = _points(RL, 1000, 96, 160)
    env = RR.proper_map(16, 32, seed=1).cuda()
    a = RL.relight_points(tracers['device'], pt, tab_d, tab_s, env, 2)
    b = RL.relight_points(tracers['device'], pt, tab_d, tab_s, env, 2)
    c = RL.relight_points(tracers['device'], pt, tab_d, tab_s, env, 2, chunk=77)
    for x, y, z in zip(a, b, c):
        assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z))
    r1 = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16), chunk=7)
    r2 = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16), chunk=1000)
    r3 = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16))
    for k in r1:
        assert torch.equal(r1[k], r2[k]) and torch.equal(r1[k], r3[k]), k
    assert float(r1['alpha'].sum()) > 100 and float(r1['rgb_lin'].max()) > 0


# ---- 7. closed forms on the device ----------------------------------------------------------------------------------------------------------
def test_a_convex_mesh_under_a_constant_map(RL):
    """nothing shadows a convex mesh: with metallic 0 the diffuse term is albedo x L0, up to the rounding of a sum of Dd equal terms in a
    fixed tree (6 butterfly levels, the partials and the division: at most 10 roundings of 2^-24 each for 64 samples), of the two
    interpolations of a constant (albedo over the triangle, the map over its texels: about 3 roundings each) and of the two products -- some
    18 roundings in the worst case, bounded here by 32 x 2^-24"""
    V, Fc = RR.scene(quad=False)
    mats = _materials(len(V), 1)
    mats['metallic'][:] = 0
    mats['albedo'][:] = np.asarray([0.8, 0.5, 0.25], np.float32)
    L0 = torch.tensor([0.5, 1.0, 3.0])
    rl = RL.Relighter(V, Fc, mats, L0.expand(4, 8, 3).contiguous(), convention='nero')
    ro, rd = rl.camera_rays(POSE, KMAT, 48, 48)
    sf = rl.surface(ro, rd)
    pt = RL.point_records(sf['pts'], -rd[sf['idx']], sf['normal'], RL.estimator_materials(sf['mat5']), None, None)
    _, dif, _ = RL.relight_points(rl.tracer, pt, RL.sample_table(64, 'cuda'), RL.sample_table(64, 'cuda'), rl.env, 0)
    want = torch.tensor([0.8, 0.5, 0.25]) * L0
    rel = float(((dif.cpu() - want) / want).abs().max())
    print(f'convex mesh, constant map: diffuse / (albedo L0) - 1 = {rel:.2e}')
    assert rel <= 32 * 2.0 ** -24
    out = rl.render(POSE, KMAT, 48, 48, samples=(64, 64))
    depth = rl.tracer.trace(ro, rd)[2]
    assert torch.equal(out['alpha'].reshape(-1) > 0, depth < 10.0) and set(out['alpha'].unique().tolist()) == {0.0, 1.0}


def test_a_point_under_a_disk(RL):
    """tests/test_relight_cpu.py compares the restatement with 1 - R^2 / (R^2 + h^2) at this sample count; here the kernel is within the
    restatement's own float32 floor, plus one sample for every ray that grazes the disk's rim by less than the margin"""
    from nero_amd.raytracing import RayTracer
    Dd, Ds, Rd, hgt = 512, 16, 0.3, 0.25
    ang = torch.linspace(0, 2 * math.pi, 257, dtype=F64)[:-1]
    V = torch.cat([torch.tensor([[0.0, 0.0, hgt]], dtype=F64), torch.stack([Rd * torch.cos(ang), Rd * torch.sin(ang), torch.full_like(ang, hgt)], -1)]).float()
    Fc = torch.stack([torch.zeros(256, dtype=torch.long), 1 + torch.arange(256), 1 + (torch.arange(256) + 1) % 256], -1)
    tr = RayTracer(V.numpy(), Fc.int().numpy())
    mat5 = torch.tensor([[0.0, 0.5, 0.8, 0.6, 0.4]])
    pt = RL.point_records(torch.zeros(1, 3).cuda(), torch.tensor([[0.3, 0.1, 1.0]]).cuda(), torch.tensor([[0.0, 0.0, 1.0]]).cuda(), mat5.cuda(),
                          torch.tensor([0.37]).cuda(), torch.tensor([0.11]).cuda())
    env = torch.full((4, 8, 3), 2.0)
    tab_d, tab_s = RR.sample_table(Dd), RR.sample_table(Ds)
    _, dif, _ = RL.relight_points(tr, pt, tab_d.cuda(), tab_s.cuda(), env.cuda(), 2)
    ref = {}
    for dt in (F32, F64):
        p = pt.cpu().to(dt)
        w, o = R.dirs(p, tab_d.to(dt), tab_s.to(dt))
        blocked, dec = RR.occluded(V.to(dt), Fc, o, w)
        dead, _ = R.dead_rays(p, w, Dd, Ds, 0)
        ref[dt] = (RR.relight(p, w, blocked, dead, env, 2, None, 0.0, Dd, Ds, 0)[1], dec)
    grazing = int((ref[F64][1]['shadow'][1][:Dd] < RR.MARGIN).sum())
    floor, err = RR.floors_and_errors(dif.cpu(), ref[F32][0], ref[F64][0], 2.0)
    floor, err = max(float(floor.max()), ULP), float(err.max())
    closed = float((dif.cpu()[0] / (mat5[0, 2:5] * 2.0)).mean())
    print(f'point under a disk: lit fraction {closed:.4f} (closed form {1 - Rd ** 2 / (Rd ** 2 + hgt ** 2):.4f}); floor {floor:.2e} kernel {err:.2e} '
          f'({err / floor:.2f} floors); {grazing} grazing rays')
    assert err <= K * floor + grazing / Dd


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ssaa', [1, 2])
def test_render(RL, mesh, relighter, ssaa):
    V, Fc = mesh
    h = w = 48
    bg = torch.tensor([0.1, 0.2, 0.3])
    out = relighter.render(POSE, KMAT, h, w, samples=(32, 32), ssaa=ssaa, seed=5, background=bg)
    plain = relighter.render(POSE, KMAT, h, w, samples=(32, 32), ssaa=ssaa, seed=5)
    Ks = np.diag([ssaa, ssaa, 1.0]).astype(np.float32) @ KMAT
    ro, rd = relighter.camera_rays(POSE, Ks, ssaa * h, ssaa * w)
    hit = (relighter.tracer.trace(ro, rd)[2] < 10.0).float().reshape(h, ssaa, w, ssaa).mean((1, 3))
    assert torch.equal(out['alpha'][..., 0], hit) and 0.1 < float(hit.mean()) < 0.9
    miss = (hit == 0).cpu()
    assert torch.equal(out['rgb_lin'].cpu()[miss], bg.expand(int(miss.sum()), 3)) and not plain['rgb_lin'].cpu()[miss].any()
    assert out['rgba8'].dtype == torch.uint8 and tuple(out['rgba8'].shape) == (h, w, 4)
    assert torch.equal(out['rgba8'][..., 3].cpu(), torch.round(hit.cpu() * 255).to(torch.uint8))
    for k, ch in (('rgb_lin', 3), ('rgb', 3), ('alpha', 1), ('albedo', 3), ('metallic', 1), ('roughness', 1), ('normal', 3), ('depth', 1)):
        assert tuple(out[k].shape) == (h, w, ch) and out[k].is_cuda and bool(torch.isfinite(out[k]).all()), k
    assert float(out['rgb'].min()) >= 0 and float(out['rgb'].max()) <= 1 and bool((out['depth'].cpu()[miss] == 10.0).all())
    if ssaa != 1:
        return
    # a few pixels against the restatement, from the camera ray on: brute-force hit, interpolation, record, rays, shadows, lookup, estimator
    Dd = Ds = 32
    tab = RR.sample_table(32)
    ref, picked = {}, None
    for dt in (F64, F32):
        o, d = RR.camera_rays(POSE, KMAT, h, w, dt)
        depth, face, bary, margin = RR.closest_hit(V.to(dt), Fc, o, d)
        if picked is None:
            cand = torch.nonzero((face >= 0) & (margin > 1e-3))[:, 0]
            picked = cand[torch.linspace(0, len(cand) - 1, 12).long()]
        f, b = face[picked], bary[picked]
        corner = V.to(dt)[Fc[f]]
        n = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
        n = torch.where((n * d[picked]).sum(-1, keepdim=True) > 0, -n, n)
        mat5 = RR.interpolate(relighter.mat5.cpu().to(dt), Fc, f, b)
        mat5 = torch.cat([mat5[:, :1], mat5[:, 1:2] ** 2, mat5[:, 2:]], -1)
        rd_, rs_ = RL.pixel_rotations(picked, 5)
        pt, dec_p = R.point_setup(RR.interpolate(V.to(dt), Fc, f, b), -d[picked], n, mat5, rd_.to(dt), rs_.to(dt))
        wd, od = R.dirs(pt, tab.to(dt), tab.to(dt))
        blocked, dec_s = RR.occluded(V.to(dt), Fc, od, wd)
        dead, _ = R.dead_rays(pt, wd, Dd, Ds, 0)
        rgb = RR.relight(pt, wd, blocked, dead, relighter.env.cpu(), 2, None, 0.0, Dd, Ds, 0)[0]
        ref[dt] = (rgb, dec_s['shadow'][1].reshape(len(picked), -1).min(-1)[0], torch.minimum(dec_p['ortho_n'][1], dec_p['ortho_r'][1]))
    ok = (ref[F64][1] > RR.MARGIN) & (ref[F64][2] > 1e-3)                               # no grazing shadow ray, no tie in a frame's choice
    got = out['rgb_lin'].reshape(-1, 3)[picked.cuda()].cpu()
    floor, err = RR.floors_and_errors(got, ref[F32][0], ref[F64][0], float(relighter.env.mean()))
    floor = max(float(floor[ok].max()), ULP)
    print(f'render: {int(ok.sum())} of {len(picked)} pixels compared; floor {floor:.2e} kernel {float(err[ok].max()):.2e} '
          f'({float(err[ok].max()) / floor:.2f} floors)')
    assert int(ok.sum()) >= 6 and float(err[ok].max()) <= K * floor


def test_the_material_renderer_relights_its_mesh(RL):
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import build_material_case, golden_mesh, load_golden
    _, meta = load_golden('mat_bell')
    ref = build_material_case(meta)
    net = NeROMaterialRenderer({'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell'}, mesh=golden_mesh())
    net.load_state_dict(ref.state_dict())
    net = net.cuda()
    env = RR.proper_map(8, 16, seed=4)
    rl = net.relight(env)
    assert rl.tracer is net.ray_tracer and rl.geometry_type == 0
    v = torch.from_numpy(net.ray_tracer._v).cuda()
    mats = net.predict_materials_of_vertices(v)
    want = torch.from_numpy(np.concatenate([mats['metallic'], mats['roughness'], mats['albedo']], -1)).cuda()
    assert torch.equal(rl.mat5, want)                                                # perceptual roughness, as predicted: not squared here
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(3, 0.0, 30.0, 2.0))[1]
    out = rl.render(pose, RL.default_K(32, 32), 32, 32, samples=(16, 16))
    hit = out['alpha'][..., 0] > 0
    assert 50 < int(hit.sum()) < 1000 and bool(torch.isfinite(out['rgb_lin']).all()) and float(out['rgb_lin'][hit].min()) >= 0
    assert float(out['rgb_lin'][hit].max()) > 0
    same = RL.Relighter(v, net.ray_tracer._f, mats, env, build='host').render(pose, RL.default_K(32, 32), 32, 32, samples=(16, 16))
    for k in out:
        assert torch.equal(out[k], same[k]), k


def test_the_script_writes_an_orbit_of_rgba_pngs(RL, mesh, tmp_path):
    from nero_amd.envlight import write_hdr
    from nero_amd.mesh import write_ply
    from nero_amd.texture import read_png
    V, Fc = mesh
    write_ply(str(tmp_path / 'm.ply'), V.numpy(), Fc.numpy())
    mats = _materials(len(V), 2)
    os.makedirs(tmp_path / 'mat')
    for k, a in mats.items():
        np.save(tmp_path / 'mat' / f'{k}.npy', a)
    env = RR.proper_map(8, 16, seed=6)
    write_hdr(str(tmp_path / 'e.hdr'), env.numpy())
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'relight.py'), '--mesh', str(tmp_path / 'm.ply'), '--material', str(tmp_path / 'mat'),
           '--hdr', str(tmp_path / 'e.hdr'), '--name', 'orbit', '--out', str(tmp_path / 'out'), '--num', '2', '--width', '32', '--height', '32',
           '--samples', '16', '16', '--cam_dist', '2.0']
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / 'out' / 'orbit')) == ['0.png', '1.png']
    rl = RL.Relighter(V, Fc, mats, str(tmp_path / 'e.hdr'))
    poses = RL.poses_in_mesh_frame(RL.relighting_poses(2, 0.0, 30.0, 2.0))
    for k in range(2):
        img = read_png(str(tmp_path / 'out' / 'orbit' / f'{k}.png'))
        want = rl.render(poses[k], RL.default_K(32, 32), 32, 32, samples=(16, 16))['rgba8'].cpu().numpy()
        assert img.shape == (32, 32, 4) and np.array_equal(img[..., 3], want[..., 3]) and 50 < int((img[..., 3] > 0).sum()) < 1000
        assert np.array_equal(img, want)
