"""GPU tier of the relighter's third strategy: the light table (nero_env_cdf), the sample set (nero_relight_mis_rays) and the fused MIS kernel
(nero_bvh_relight_mis) against the restatement (tests/envsample_ref.py), reproducibility, a constant map, and the Python layer end to end.

Tolerances are those of tests/test_relight_gpu.py: K_FLOOR (4) x the distance between the restatement evaluated in float32 and in float64 on
the same inputs, relative to max(|value|, a scale of the quantity), pooled per condition class.  Everything integer -- the running sum from
the kernel's own float weights, the drawn cells -- is compared exactly.  Every test prints its kernel / floor ratio before it asserts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import envsample_ref as ER
from tests import relight_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
K = RR.K_FLOOR
ULP = 2.0 ** -23
POSE = RR.relighting_poses(4, 30.0, 60.0, 2.4)[1].numpy()
KMAT = np.asarray([[60.0, 0, 24], [0, 60.0, 24], [0, 0, 1]], np.float32)


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
def tracer(RL, mesh):
    from nero_amd.raytracing import RayTracer
    V, Fc = mesh
    return RayTracer(V.cuda(), Fc.int().cuda(), build='device')


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------
def _table_case(RL, env, conv, rot, clamp, keep=None):
    """build twice; the running sum from the kernel's own weights, info, the weights against the restatement -> floor, err"""
    t1 = RL.light_table(env.cuda(), conv, rot, clamp, weights=True)
    t2 = RL.light_table(env.cuda(), conv, rot, clamp, weights=True)
    assert torch.equal(t1.cdf, t2.cdf) and torch.equal(t1.info, t2.info) and torch.equal(_bits(t1.weights), _bits(t2.weights))
    a_dev, cdf, info = t1.weights.cpu(), t1.cdf.cpu().numpy(), t1.info.cpu().numpy()
    a32, fb = ER.weights(env, conv, rot, clamp or 0.0, F32)
    a64, fb64 = ER.weights(env, conv, rot, clamp or 0.0, F64)
    assert fb == fb64 and bool(torch.isfinite(a_dev).all()) and float(a_dev.min()) >= 0
    want_cdf, want_info = ER.table_from_weights(a_dev.numpy(), fb)
    assert np.array_equal(cdf, want_cdf) and np.array_equal(info, want_info), (info, want_info)
    assert info[0] == cdf[-1] > 0 and cdf[-1] <= 2 ** 62 and info[3] == ER.weight_bits(len(cdf))
    floor, err = RR.floors_and_errors(a_dev[:, None], a32[:, None], a64[:, None], float(a64.mean()))
    if keep is not None:
        floor, err = floor[keep], err[keep]
    return max(float(floor.max()), ULP), float(err.max())


@pytest.mark.parametrize('hw', [(1, 1), (1, 2), (3, 5), (16, 32), (64, 128)])
def test_light_table(RL, hw):
    h, w = hw
    env = RR.proper_map(h, w, hot=(h // 2, w // 2, 1000.0))
    for conv in (0, 1, 2):
        for rot in (None, RR.ROT):
            for clamp in (None, 1.0):
                floor, err = _table_case(RL, env, conv, rot, clamp)
                print(f'light table {h}x{w} conv {conv} rot {rot is not None} clamp {clamp}: floor {floor:.2e} kernel {err:.2e} ({err / floor:.2f} floors)')
                assert err <= K * floor


def test_light_table_of_a_map_with_bad_texels(RL):
    env = RR.proper_map(16, 32, seed=3, hot=(5, 9, 1000.0))
    env[2, 4], env[9, 20], env[12, 7] = float('nan'), float('inf'), -5.0
    bad = torch.zeros(16, 32, dtype=torch.bool)
    for r, c in ((2, 4), (9, 20), (12, 7)):                            # the cells whose nine lookups can touch a bad texel
        bad[max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] = True
    floor, err = _table_case(RL, env, 2, None, None, keep=~bad.reshape(-1))
    print(f'light table with NaN, inf and negative texels: floor {floor:.2e} kernel {err:.2e} ({err / floor:.2f} floors)')
    assert err <= K * floor


def test_a_black_map_takes_the_fallback(RL):
    for h, w in ((1, 1), (5, 7), (16, 32)):
        env = torch.zeros(h, w, 3)
        floor, err = _table_case(RL, env, 2, None, None)
        t = RL.light_table(env.cuda(), 2, weights=True)
        info = t.info.cpu().numpy()
        assert info[4] == 1 and info[2] == 0 and info[1] == 0 and float(t.weights.min()) > 0
        print(f'black {h}x{w}: fallback weights floor {floor:.2e} kernel {err:.2e} ({err / floor:.2f} floors)')
        assert err <= K * floor
    nan = torch.full((4, 8, 3), float('nan'))
    assert int(RL.light_table(nan.cuda(), 2).info[4]) == 1


def _v_of(w):
    PI = ER._pi(w.dtype)[0]
    return torch.atan2(w[:, 2], torch.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1])) / PI + 0.5


# ---- 2. the sample set ----------------------------------------------------------------------------------------------------------------------
def _case(RL, P_, Dd, Ds, Dl, i):
    c, tab_d, tab_s, tab_l = ER.candidates(P_, Dd, Ds, Dl)
    pt = RL.point_records(c['pts'].cuda(), c['view'].cuda(), c['normals'].cuda(), c['mat5'].cuda(), c['rand_d'].cuda(), c['rand_s'].cuda())
    env, conv, rot, clamp = ER.env_of_case(i)
    table = RL.light_table(env.cuda(), conv, rot, clamp)
    return c, pt, tab_d.cuda(), tab_s.cuda(), tab_l.cuda(), env, conv, rot, clamp, table


@pytest.mark.parametrize('Dd,Ds,Dl', ER.MIS_CASES)
def test_mis_rays(RL, Dd, Ds, Dl):
    P_, D = 65, Dd + Ds + Dl
    c, pt, tab_d, tab_s, tab_l, env, conv, rot, clamp, table = _case(RL, P_, Dd, Ds, Dl, Dd + Dl)
    cdf = table.cdf.cpu().numpy()
    for geom, rand_l in ((0, c['rand_l']), (1, None)):
        ro, rd, dead, cell, pdf = RL.relight_mis_rays(pt, tab_d, tab_s, tab_l, table, None if rand_l is None else rand_l.cuda(), geom)
        ro2, rd2, dead2 = RL.relight_rays(pt, tab_d, tab_s, geom)
        first = lambda t, n=3: t.reshape(P_, D, -1)[:, :Dd + Ds].reshape(-1, n)
        assert torch.equal(_bits(first(ro)), _bits(ro2)) and torch.equal(_bits(first(rd)), _bits(rd2))      # relight_ray's, bit for bit
        assert torch.equal(first(dead, 1).reshape(-1), dead2)
        p = pt.cpu()
        ref = {dt: ER.mis_rays(p.to(dt), tab_d.cpu(), tab_s.cpu(), tab_l.cpu(), rand_l, cdf, table.gh, table.gw, geom) for dt in (F32, F64)}
        w64, o64, _, cell64, pdf64, _, is_light = ref[F64]
        w32, o32, _, cell32, pdf32, _, _ = ref[F32]
        cell, pdf, rd, ro, dead = cell.cpu().numpy(), pdf.cpu(), rd.cpu(), ro.cpu(), dead.cpu().bool()
        il, lt = is_light, is_light.numpy()
        assert np.array_equal(cell[lt], cell64[lt]) and np.array_equal(cell32[lt], cell64[lt])               # the integer inversion: exact
        assert cell.min() >= 0 and cell.max() < table.gh * table.gw
        # the looked-up cell and the density of the other strategies' samples: restated from the KERNEL's directions (checked bit for bit
        # above, and against float64 in tests/test_relight_gpu.py) -- at the roughness floor a GGX direction is itself only good to 3e-5
        margin = torch.ones(P_ * D, dtype=F64)
        cell32, cell64, pdf32, pdf64 = cell32.copy(), cell64.copy(), pdf32.clone(), pdf64.clone()
        for dt, cc, pp in ((F32, cell32, pdf32), (F64, cell64, pdf64)):
            cb, vb, mb = ER.lookup_cell(rd[~il].to(dt), table.gh, table.gw)
            cc[~lt] = cb
            pp[~il] = ER.pdf_light(cdf, table.gh, table.gw, cb, vb)
            if dt == F64:
                margin[~il] = mb
        ex = (margin < RR.MARGIN).numpy()
        assert ex.mean() <= RR.CAP and not ex[lt].any()
        assert np.array_equal(cell[~ex], cell64[~ex]), int((cell[~ex] != cell64[~ex]).sum())
        floor_w = max(float((w32.double() - w64)[il].abs().max()), float((o32.double() - o64)[il].abs().max()), ULP)
        err_w = max(float((rd.double() - w64)[il].abs().max()), float((ro.double() - o64)[il].abs().max()))
        same = torch.from_numpy(~ex & (cell32 == cell64))
        # p_l divides by cos(el): one rounding of v moves it by tan(el) times as much, so floor and error are taken relative to that
        # condition number too -- a ray next to the grid's axis then counts like any other, and the pooled floor is no accident of which
        # of a few hundred rays points there
        f_p, e_p = RR.floors_and_errors(pdf[:, None], pdf32[:, None], pdf64[:, None], 1.0 / (4 * math.pi))
        cond = 1.0 + torch.tan(((_v_of(rd.double()) - 0.5) * math.pi).abs().clamp(max=math.pi / 2 - 1e-6))
        f_p, e_p = f_p / cond, e_p / cond
        floor_p, err_p = max(float(f_p[same].max()), ULP), float(e_p[same].max())
        nw = (p[:, None, 3:6].double() * rd.double().reshape(P_, D, 3)).sum(-1)
        dead64 = ((torch.arange(D) >= Dd)[None, :] & (nw < -1e-6) & (geom == 0)).reshape(-1)
        close = ((nw + 1e-6).abs() < RR.MARGIN).reshape(-1)
        print(f'mis_rays ({Dd},{Ds},{Dl}) geom {geom}: light directions floor {floor_w:.2e} kernel {err_w:.2e} ({err_w / floor_w:.2f} floors); '
              f'pdf_l floor {floor_p:.2e} kernel {err_p:.2e} ({err_p / floor_p:.2f} floors); {int(ex.sum())} of {len(ex)} rays exempt; '
              f'{int(dead.sum())} dead, {int((dead != dead64).sum())} differ, {int(close.sum())} within the margin')
        assert err_w <= K * floor_w and err_p <= K * floor_p
        assert bool(torch.isfinite(pdf).all()) and float(pdf.min()) >= 0
        assert not bool(((dead != dead64) & ~close).any())
        if geom == 1:
            assert not bool(dead.any())
        else:
            assert not bool(dead.reshape(P_, D)[:, :Dd].any())


# ---- 3. fused = composed --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fused(RL, tracer):
    """every case once: the kernel's own rays and cells (nero_relight_mis_rays), nero_bvh_occluded on them, the restatement in float32 and
    float64 from those -> {(Dd, Ds, Dl, P, geom): (floor [P], err [P], class key [P], lit, finite)} for rgb, diffuse and specular together"""
    out = {}
    for i, (Dd, Ds, Dl) in enumerate(ER.MIS_CASES):
        for P_ in ER.MIS_P:
            c, pt, tab_d, tab_s, tab_l, env, conv, rot, clamp, table = _case(RL, P_, Dd, Ds, Dl, i + P_)
            cdf = table.cdf.cpu().numpy()
            rand_l = c['rand_l'].cuda()
            for geom in (0, 1):
                got = RL.relight_points(tracer, pt, tab_d, tab_s, env.cuda(), conv, rot, clamp, geom, tab_l=tab_l, rand_l=rand_l, table=table)
                ro, rd, dead, cell, _ = RL.relight_mis_rays(pt, tab_d, tab_s, tab_l, table, rand_l, geom)
                blocked = tracer.occluded(ro, rd, skip=dead).bool().cpu()
                dead, w, p, cell = dead.bool().cpu(), rd.cpu(), pt.cpu(), cell.cpu().numpy()
                ref = []
                for dt in (F32, F64):
                    pdf = ER.pdf_light(cdf, table.gh, table.gw, cell, _v_of(w.to(dt)))
                    ref.append(ER.relight_mis(p.to(dt), w.to(dt), blocked, dead, pdf, env, conv, rot, clamp or 0.0, Dd, Ds, Dl, geom))
                scale = float(env.mean())
                fe = [RR.floors_and_errors(got[k].cpu(), ref[0][k], ref[1][k], scale) for k in range(3)]
                floor = torch.stack([f for f, _ in fe]).max(0)[0]
                err = torch.stack([e for _, e in fe]).max(0)[0]
                key = [(geom, int(x), Dd + Ds + Dl < 16) for x in c['cls']]
                lit = float((~(blocked | dead)).float().mean())
                out[(Dd, Ds, Dl, P_, geom)] = (floor, err, key, lit, all(bool(torch.isfinite(g).all()) for g in got))
    pooled = {}
    for floor, _, key, _, _ in out.values():
        for f, k in zip(floor.tolist(), key):
            pooled[k] = max(pooled.get(k, ULP), f)
    return out, pooled


@pytest.mark.parametrize('geom', [0, 1])
@pytest.mark.parametrize('P_', ER.MIS_P)
@pytest.mark.parametrize('Dd,Ds,Dl', ER.MIS_CASES)
def test_fused_equals_composed(fused, Dd, Ds, Dl, P_, geom):
    out, pooled = fused
    floor, err, key, lit, finite = out[(Dd, Ds, Dl, P_, geom)]
    assert finite
    ratio = {}
    for e, k in zip(err.tolist(), key):
        ratio[k] = max(ratio.get(k, 0.0), e / pooled[k])
    print(f'fused ({Dd},{Ds},{Dl}) P {P_} geom {geom}: {lit:.0%} of the rays lit; kernel / pooled float32 floor per (geom, class, D < 16): '
          + ', '.join(f'{k}: {v:.2f} (floor {pooled[k]:.1e})' for k, v in sorted(ratio.items())))
    assert max(ratio.values()) <= K


# ---- 4. reproducibility ---------------------------------------------------------------------------------------------------------------------
def _materials(nV, seed=0):
    g = np.random.default_rng(seed)
    return {'metallic': g.uniform(0, 1, (nV, 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (nV, 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (nV, 3)).astype(np.float32)}


@pytest.fixture(scope='module')
def relighter(RL, mesh, tracer):
    V, Fc = mesh
    env = RR.proper_map(16, 32, seed=2, hot=(5, 9, 1000.0))
    return RL.Relighter(V, Fc, _materials(len(V)), env, convention='blender', tracer=tracer)


def test_the_same_bits_on_every_run_for_every_chunk_and_for_both_walks(RL, L, tracer, relighter):
    c, pt, tab_d, tab_s, tab_l, env, conv, rot, clamp, table = _case(RL, 1000, 96, 160, 200, 4)
    rand_l = c['rand_l'].cuda()
    run = lambda **kw: RL.relight_points(tracer, pt, tab_d, tab_s, env.cuda(), conv, rot, clamp, 0, tab_l=tab_l, rand_l=rand_l, table=table, **kw)
    a, b, d = run(), run(), run(chunk=77)
    e = RL.relight_points(tracer, pt, tab_d, tab_s, env.cuda(), conv, rot, clamp, 0, tab_l=tab_l, rand_l=rand_l)       # the table built inside
    walks = {}
    for mode in (0, 1):
        L.check(L.lib.nero_bvh_set_traversal(tracer._handle(), mode))
        walks[mode] = run()
    for k in range(3):
        for other in (b, d, e, walks[0], walks[1]):
            assert torch.equal(_bits(a[k]), _bits(other[k])), k
    r1 = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16, 32), chunk=7)
    r2 = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16, 32), chunk=1000)
    r3 = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16, 32))
    for k in r1:
        assert torch.equal(r1[k], r2[k]) and torch.equal(r1[k], r3[k]), k
    assert float(r1['alpha'].sum()) > 100 and float(r1['rgb_lin'].max()) > 0
    assert len(relighter._light) == 1 and relighter.light_table(None) is relighter.light_table(0.0)                     # cached per cap
    assert relighter.light_table(50.0) is not relighter.light_table(None)


# ---- 5. a constant map ----------------------------------------------------------------------------------------------------------------------
CONSTANT_MAP_DISTANCE = 0.041     # 2.03e-2 measured on the CPU (tests/test_relight_mis_cpu.py::test_the_restatement_under_a_constant_map), times 2


def test_a_convex_mesh_under_a_constant_map(RL):
    """nothing shadows a convex mesh: with metallic 0 the diffuse term estimates albedo x L0.  The kernel is within the float32 floor of the
    restatement on its own rays; the restatement in float64 is within CONSTANT_MAP_DISTANCE of albedo L0 -- the quadrature error of 64 + 64
    + 64 lattice samples under the mixture, measured on the CPU side at 2.03e-2 and doubled for the fixed lattice, not tuned to the kernel"""
    V, Fc = RR.scene(quad=False)
    mats = _materials(len(V), 1)
    mats['metallic'][:] = 0
    mats['albedo'][:] = np.asarray([0.8, 0.5, 0.25], np.float32)
    L0 = torch.tensor([0.5, 1.0, 3.0])
    env = L0.expand(4, 8, 3).contiguous()
    rl = RL.Relighter(V, Fc, mats, env, convention='nero')
    ro, rd = rl.camera_rays(POSE, KMAT, 48, 48)
    sf = rl.surface(ro, rd)
    idx = sf['idx']
    pt = RL.point_records(sf['pts'], -rd[idx], sf['normal'], RL.estimator_materials(sf['mat5']), *RL.pixel_rotations(idx, 0))
    tabs = [RL.sample_table(64, 'cuda') for _ in range(3)]
    rand_l = RL.pixel_shifts(idx, 0)
    table = rl.light_table(None)
    _, dif, _ = RL.relight_points(rl.tracer, pt, tabs[0], tabs[1], rl.env, 0, tab_l=tabs[2], rand_l=rand_l, table=table)
    o, w, dead, cell, _ = RL.relight_mis_rays(pt, tabs[0], tabs[1], tabs[2], table, rand_l, 0)
    # (a light sample may graze the facet it starts from: the float32 hit point lies a few 1e-8 off the facet's plane, and a ray that rises by
    #  less than that over the facet's width meets it again.  Such a ray carries NoL < 1e-3; the restatement takes the tracer's word for it)
    blocked = rl.tracer.occluded(o, w, skip=dead).bool().cpu()
    w, dead, cell, p = w.cpu(), dead.bool().cpu(), cell.cpu().numpy(), pt.cpu()
    grazing = int((blocked & ~dead).sum())
    cdf = table.cdf.cpu().numpy()
    ref = [ER.relight_mis(p.to(dt), w.to(dt), blocked, dead, ER.pdf_light(cdf, 4, 8, cell, _v_of(w.to(dt))), env, 0, None, 0.0, 64, 64, 64, 0)[1]
           for dt in (F32, F64)]
    floor, err = RR.floors_and_errors(dif.cpu(), ref[0], ref[1], float(env.mean()))
    floor, err = max(float(floor.max()), ULP), float(err.max())
    want = torch.tensor([0.8, 0.5, 0.25], dtype=F64) * L0.double()
    rel = float(((ref[1] - want) / want).abs().max())
    assert grazing <= 0.001 * len(w)
    print(f'convex mesh, constant map: {grazing} of {len(w)} rays graze their own facet; kernel vs restatement floor {floor:.2e} kernel {err:.2e} ({err / floor:.2f} floors); restatement / '
          f'(albedo L0) - 1 = {rel:.2e}')
    assert err <= K * floor and rel <= CONSTANT_MAP_DISTANCE


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------------------
def test_mis_beats_the_two_strategies_at_equal_sample_count(relighter):
    """48 x 48 under the hot-texel map, no clamp: against a (2048, 2048) two-strategy render the linear RMSE over the hit pixels of samples =
    (16, 16, 32) is below that of samples = (32, 32); coverage, depth and the material planes do not depend on the path"""
    truth = relighter.render(POSE, KMAT, 48, 48, samples=(2048, 2048))
    two = relighter.render(POSE, KMAT, 48, 48, samples=(32, 32))
    mis = relighter.render(POSE, KMAT, 48, 48, samples=(16, 16, 32))
    hit = truth['alpha'][..., 0] > 0
    rmse = lambda x: float(torch.sqrt(((x['rgb_lin'] - truth['rgb_lin'])[hit] ** 2).mean()))
    print(f'RMSE over {int(hit.sum())} hit pixels against (2048, 2048): (32, 32) {rmse(two):.4f}, (16, 16, 32) {rmse(mis):.4f}; mean radiance '
          f'{float(truth["rgb_lin"][hit].mean()):.4f}')
    assert int(hit.sum()) > 100 and rmse(mis) < rmse(two)
    for k in ('alpha', 'depth', 'albedo', 'metallic', 'roughness', 'normal'):
        assert torch.equal(two[k], mis[k]), k
    assert bool(torch.isfinite(mis['rgb_lin']).all()) and float(mis['rgb_lin'][hit].min()) >= 0
    with pytest.raises(ValueError):
        relighter.render(POSE, KMAT, 8, 8, samples=(16,))


def test_the_script_takes_a_third_sample_count(RL, mesh, tmp_path):
    from nero_amd.envlight import write_hdr
    from nero_amd.mesh import write_ply
    from nero_amd.texture import read_png
    V, Fc = mesh
    write_ply(str(tmp_path / 'm.ply'), V.numpy(), Fc.numpy())
    mats = _materials(len(V), 2)
    os.makedirs(tmp_path / 'mat')
    for k, a in mats.items():
        np.save(tmp_path / 'mat' / f'{k}.npy', a)
    write_hdr(str(tmp_path / 'e.hdr'), RR.proper_map(8, 16, seed=6, hot=(2, 5, 300.0)).numpy())
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'relight.py'), '--mesh', str(tmp_path / 'm.ply'), '--material', str(tmp_path / 'mat'),
           '--hdr', str(tmp_path / 'e.hdr'), '--name', 'orbit', '--out', str(tmp_path / 'out'), '--num', '2', '--width', '32', '--height', '32',
           '--samples', '16', '16', '32', '--cam_dist', '2.0']
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert '16+16+32' in run.stdout and sorted(os.listdir(tmp_path / 'out' / 'orbit')) == ['0.png', '1.png']
    rl = RL.Relighter(V, Fc, mats, str(tmp_path / 'e.hdr'))
    poses = RL.poses_in_mesh_frame(RL.relighting_poses(2, 0.0, 30.0, 2.0))
    for k in range(2):
        img = read_png(str(tmp_path / 'out' / 'orbit' / f'{k}.png'))
        want = rl.render(poses[k], RL.default_K(32, 32), 32, 32, samples=(16, 16, 32))['rgba8'].cpu().numpy()
        assert img.shape == (32, 32, 4) and 50 < int((img[..., 3] > 0).sum()) < 1000 and np.array_equal(img, want)
        two = rl.render(poses[k], RL.default_K(32, 32), 32, 32, samples=(16, 16))['rgba8'].cpu().numpy()
        assert np.array_equal(img[..., 3], two[..., 3]) and not np.array_equal(img, two)
