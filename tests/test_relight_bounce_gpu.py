"""GPU tier of the relighter's one bounce: what every lane decides (nero_relight_bounce_rays) against the entry points it is composed of, the
fused kernels (nero_bvh_relight_bounce, nero_bvh_relight_mis_bounce) against the restatement (tests/bounce_ref.py) evaluated on the device's
own discrete facts, reproducibility, a convex mesh, a face that names a vertex the mesh does not have, and the Python layer end to end.

Tolerances are those of tests/test_relight_gpu.py: K_FLOOR (4) x the distance between the restatement evaluated in float32 and in float64 on
the same inputs, relative to max(|value|, mean map radiance) and pooled per (geometry type, point class, D < 16).  Everything discrete --
faces, (u, v), states, strategies -- is compared exactly.  Every test prints its kernel / floor ratio before it asserts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bounce_ref as B
from tests import envsample_ref as ER
from tests import mc_shade_ref as R
from tests import relight_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
from tests.test_relight_gpu import K, KMAT, POSE, ULP  # noqa: E402  (tests/test_relight_gpu.py's own K; the camera of its render tests)

CASES = B.cases()


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
def tracers(RL):
    from nero_amd.raytracing import RayTracer

    class SmallTracer(RayTracer):
        """RayTracer refuses a mesh of eight triangles or fewer (the reference wrapper's guard); the library builds the corner's six"""

        def __init__(self, vertices, triangles):
            self.build, self._h, self._dv, self._df = 'host', None, None, None
            self._host = (np.ascontiguousarray(vertices.numpy(), dtype=np.float32), np.ascontiguousarray(triangles.numpy(), dtype=np.int32))

    out = {'corner': SmallTracer(*B.corner_scene()[:2])}
    for name, (V, Fc) in (('sphere', RR.scene(3)), ('convex', RR.scene(3, quad=False))):
        out[name] = RayTracer(V.cuda(), Fc.int().cuda(), build='device')
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _v_of(w):
    PI = ER._pi(w.dtype)[0]
    return torch.atan2(w[:, 2], torch.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1])) / PI + 0.5


def _device_case(RL, tr, i, P_, Dd, Ds, Dl, mesh):
    s = B.case_inputs(i, P_, Dd, Ds, Dl, mesh)
    c = s['c']
    cu = lambda t: None if t is None else t.cuda()
    s['pt'] = RL.point_records(c['pts'].cuda(), c['view'].cuda(), c['normals'].cuda(), c['mat5'].cuda(), c['rand_d'].cuda(), c['rand_s'].cuda())
    s['mesh_dev'] = (s['V'].cuda(), s['Fc'].int().cuda(), s['vmat5'].cuda(), cu(s['normals']))
    s['key_dev'] = torch.from_numpy(s['key']).cuda()
    s['table'] = RL.light_table(s['env'].cuda(), s['conv'], s['rot'], s['clamp']) if Dl else None
    s['mis'] = dict(tab_l=s['tab_l'].cuda(), rand_l=c['rand_l'].cuda(), table=s['table']) if Dl else {}
    return s


def _run(RL, tr, s, geom, **kw):
    """the fused kernel with one bounce -> rgb, diffuse, spec, indirect"""
    return RL.relight_points(tr, s['pt'], s['tab_d'].cuda(), s['tab_s'].cuda(), s['env'].cuda(), s['conv'], s['rot'], s['clamp'], geom, bounces=1,
                             mesh=s['mesh_dev'], key=s['key_dev'], **s['mis'], **kw)


# ---- every case once ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs(RL, L, tracers):
    """per case: the lanes' decisions under both walks, the entry points they are composed of, the fused outputs, and the restatement in
    float32 and float64 from the device's discrete facts -> {case index: dict}, pooled floors per (geom, class, D < 16)"""
    out = {}
    for (i, P_, Dd, Ds, Dl, mesh, geom) in CASES:
        tr = tracers[mesh]
        D = Dd + Ds + Dl
        s = _device_case(RL, tr, i, P_, Dd, Ds, Dl, mesh)
        r = {'P': P_, 'D': D}
        rays, fused = {}, {}
        for mode in (0, 1):
            L.check(L.lib.nero_bvh_set_traversal(tr._handle(), mode))
            rays[mode] = RL.relight_bounce_rays(tr, s['pt'], s['tab_d'].cuda(), s['tab_s'].cuda(), s['mesh_dev'], s['key_dev'], geom, **s['mis'])
            fused[mode] = _run(RL, tr, s, geom)
        r['walks_agree'] = all(torch.equal(_bits(rays[0][k]) if rays[0][k].dtype == torch.float32 else rays[0][k],
                                           _bits(rays[1][k]) if rays[1][k].dtype == torch.float32 else rays[1][k]) for k in rays[0]) \
            and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fused[0], fused[1]))
        ry, got = rays[1], fused[1]
        # the entry points the lanes are composed of
        if Dl:
            ro, rd, dead, cell1, _ = RL.relight_mis_rays(s['pt'], s['tab_d'].cuda(), s['tab_s'].cuda(), s['mis']['tab_l'], s['table'], s['mis']['rand_l'], geom)
        else:
            ro, rd, dead = RL.relight_rays(s['pt'], s['tab_d'].cuda(), s['tab_s'].cuda(), geom)
        _, face, bary = RL.trace_faces(tr, ro, rd)
        blocked = tr.occluded(ro, rd, skip=dead).bool()
        live = ~dead.bool()
        state = ry['state'].long()
        r['faces_equal'] = torch.equal(ry['face'][live], face[live]) and torch.equal(_bits(ry['bary'][live]), _bits(bary[live])) \
            and bool((ry['face'][~live] == -1).all()) and not bool(ry['bary'][~live].any())
        r['states_agree'] = torch.equal(state == 1, dead.bool()) and torch.equal(state >= 2, blocked & live) and torch.equal(state == 0, live & ~blocked) \
            and torch.equal(ry['face'] >= 0, state >= 2) and int(state.max()) <= 3
        sec = (state == 2) | (state == 3)
        u1, _, _ = B.variates(s['key'], D)
        s_np, _ = B.strategy(u1, Dd, Ds, Dl)
        want_s = torch.where(sec.cpu(), torch.from_numpy(s_np.reshape(-1)), torch.full((P_ * D,), -1, dtype=torch.long))
        r['strategy_exact'] = torch.equal(ry['strategy'].cpu().long(), want_s)
        blocked2 = tr.occluded(ry['sec_o'], ry['sec_d'], skip=(state != 2).to(torch.uint8)).bool().cpu()
        base = RL.relight_points(tr, s['pt'], s['tab_d'].cuda(), s['tab_s'].cuda(), s['env'].cuda(), s['conv'], s['rot'], s['clamp'], geom, **s['mis'])
        r['direct_equal'] = torch.equal(got[1], base[1]) and torch.equal(got[2], base[2])
        # the restatement, from the device's facts
        p, w = s['pt'].cpu(), rd.cpu()
        m = (s['V'], s['Fc'], s['vmat5'], s['normals'])
        table = (s['table'].cdf.cpu().numpy(), s['table'].gh, s['table'].gw) if Dl else None
        ref = {}
        for dt in (F32, F64):
            pdf = ER.pdf_light(table[0], table[1], table[2], cell1.cpu().numpy(), _v_of(w.to(dt))) if Dl else None
            ref[dt] = B.bounce(p.to(dt), w.to(dt), pdf, state.cpu(), ry['face'].cpu(), ry['bary'].cpu(), blocked2, s['key'], m, s['env'], s['conv'], s['rot'],
                               s['clamp'] or 0.0, Dd, Ds, Dl, geom, table, strat=ry['strategy'].cpu().numpy(),
                               cell2=ry['cell'].cpu().numpy() if Dl else None)
        ex = B.exempt(ref[F64]['dec'], B.CONTINUOUS_KEYS)
        r['exempt'] = ex
        scale = float(s['env'].mean())
        gk = {'indirect': got[3].cpu(), 'rgb': got[0].cpu()}
        fe = [RR.floors_and_errors(gk[k], ref[F32][k], ref[F64][k], scale) for k in gk]
        r['floor'], r['err'] = torch.stack([f for f, _ in fe]).max(0)[0], torch.stack([e for _, e in fe]).max(0)[0]
        r['key'] = [(geom, int(x), D < 16) for x in s['c']['cls']]
        r['finite'] = all(bool(torch.isfinite(g).all()) for g in got) and float(got[3].min()) >= 0
        r['bounced'] = float(sec.float().mean())
        r['lit2'] = float(((state.cpu() == 2) & ~blocked2).float().mean())
        # the secondary rays and their density, lane by lane (lanes of exempt points aside)
        keep = (sec.cpu() & ~ex[:, None].expand(P_, D).reshape(-1))
        r['n_sec'] = int(keep.sum())
        if r['n_sec']:
            d64, d32 = ref[F64], ref[F32]
            r['ray_floor'] = max(float((d32['sec_o'].double() - d64['sec_o'])[keep].abs().max()), float((d32['sec_d'].double() - d64['sec_d'])[keep].abs().max()), ULP)
            r['ray_err'] = max(float((ry['sec_o'].cpu().double() - d64['sec_o'])[keep].abs().max()), float((ry['sec_d'].cpu().double() - d64['sec_d'])[keep].abs().max()))
            if Dl:
                f_p, e_p = RR.floors_and_errors(ry['pdf_l'].cpu()[:, None], d32['pdf_l2'][:, None], d64['pdf_l2'][:, None], 1.0 / (4 * math.pi))
                cond = 1.0 + torch.tan(((_v_of(d64['sec_d']) - 0.5) * math.pi).abs().clamp(max=math.pi / 2 - 1e-6))   # p_l divides by cos(el)
                r['pdf_floor'], r['pdf_err'] = max(float((f_p / cond)[keep].max()), ULP), float((e_p / cond)[keep].max())
            else:
                r['pdf_zero'] = not bool(ry['pdf_l'].any()) and bool((ry['cell'] == -1).all())
            want_dead2 = d64['dead2']
            close = (d64['dec']['dead2'][1].reshape(-1) < RR.MARGIN)
            r['dead2_agree'] = not bool((((state.cpu() == 3) != want_dead2) & sec.cpu() & ~close).any())
        out[i] = r
    pooled = {}
    for r in out.values():
        for f, k, e in zip(r['floor'].tolist(), r['key'], r['exempt'].tolist()):
            if not e:
                pooled[k] = max(pooled.get(k, ULP), f)
    return out, pooled


@pytest.mark.parametrize('i,P_,Dd,Ds,Dl,mesh,geom', CASES)
def test_what_every_lane_decides(runs, i, P_, Dd, Ds, Dl, mesh, geom):
    """face and (u, v) are nero_bvh_trace_faces' on nero_relight_rays' own rays, bit for bit; the states are RayTracer.occluded's and the dead
    flags; the strategy is the numpy restatement of the hash; both walks give the same bits; secondary origins, directions and p_l are
    within K pooled float32 floors of the restatement"""
    r = runs[0][i]
    assert r['faces_equal'] and r['states_agree'] and r['strategy_exact'] and r['walks_agree']
    if mesh == 'corner' and P_ * r['D'] >= 64:
        assert r['bounced'] >= 0.2                                     # (shown on the CPU too: the test cannot pass on free rays alone)
    if not r['n_sec']:
        print(f'case {i}: no lane bounces')
        return
    txt = f'case {i} ({mesh}, P {P_}, ({Dd}, {Ds}, {Dl}), geom {geom}): {r["bounced"]:.0%} of the lanes bounce; secondary rays floor {r["ray_floor"]:.2e} ' \
          f'kernel {r["ray_err"]:.2e} ({r["ray_err"] / r["ray_floor"]:.2f} floors)'
    if Dl:
        txt += f'; p_l floor {r["pdf_floor"]:.2e} kernel {r["pdf_err"]:.2e} ({r["pdf_err"] / r["pdf_floor"]:.2f} floors)'
    print(txt)
    assert r['dead2_agree'] and r['ray_err'] <= K * r['ray_floor']
    assert r['pdf_err'] <= K * r['pdf_floor'] if Dl else r['pdf_zero']


@pytest.mark.parametrize('i,P_,Dd,Ds,Dl,mesh,geom', CASES)
def test_fused_equals_composed(runs, i, P_, Dd, Ds, Dl, mesh, geom):
    """diffuse_lin and spec_lin are the no-bounce kernel's, bit for bit; indirect_lin and rgb_lin are within K pooled floors of the
    restatement evaluated on the device's states, faces, (u, v), strategies, cells and second shadow rays; at most 2 % of the points are
    exempt (a frame tie or the flat normal's side nearer than relight_ref.MARGIN)"""
    out, pooled = runs
    r = out[i]
    assert r['finite'] and r['direct_equal']
    assert float(r['exempt'].float().mean()) <= RR.CAP
    ratio = {}
    for e, k, ex in zip(r['err'].tolist(), r['key'], r['exempt'].tolist()):
        if not ex:
            ratio[k] = max(ratio.get(k, 0.0), e / pooled[k])
    print(f'case {i} ({mesh}, P {P_}, ({Dd}, {Ds}, {Dl}), geom {geom}): {r["bounced"]:.0%} of the lanes bounce, {r["lit2"]:.0%} fetch light there, '
          f'{int(r["exempt"].sum())} points exempt; kernel / pooled float32 floor per (geom, class, D < 16): '
          + ', '.join(f'{k}: {v:.2f} (floor {pooled[k]:.1e})' for k, v in sorted(ratio.items())))
    assert not ratio or max(ratio.values()) <= K


# ---- reproducibility ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Dl', [0, 32])
def test_the_same_bits_on_every_run_for_every_chunk_and_for_both_walks(RL, L, tracers, Dl):
    tr = tracers['corner']
    Dd, Ds = (96, 160) if Dl == 0 else (16, 16)
    s = _device_case(RL, tr, 3, 1000, Dd, Ds, Dl, 'corner')
    a, b = _run(RL, tr, s, 0), _run(RL, tr, s, 0)
    others = [b] + [_run(RL, tr, s, 0, chunk=ch) for ch in (1, 63, 1000)]
    for mode in (0, 1):
        L.check(L.lib.nero_bvh_set_traversal(tr._handle(), mode))
        others.append(_run(RL, tr, s, 0))
    for o in others:
        for k in range(4):
            assert torch.equal(_bits(a[k]), _bits(o[k])), k
    assert float(a[3].max()) > 0 and torch.equal(a[0], (a[1] + a[2]) + a[3])


# ---- a convex mesh --------------------------------------------------------------------------------------------------------------------------
def test_no_indirect_light_on_a_convex_mesh(RL, tracers):
    """camera-visible points of the plain icosphere: a point none of whose lanes meets the mesh has indirect_lin exactly 0 and rgb_lin the
    no-bounce kernel's bits"""
    V, Fc = RR.scene(3, quad=False)
    mats = {'metallic': np.full((len(V), 1), 0.3, np.float32), 'roughness': np.full((len(V), 1), 0.5, np.float32),
            'albedo': np.full((len(V), 3), 0.6, np.float32)}
    rl = RL.Relighter(V, Fc, mats, RR.proper_map(16, 32, seed=5), convention='blender', tracer=tracers['convex'])
    ro, rd = rl.camera_rays(POSE, KMAT, 48, 48)
    sf = rl.surface(ro, rd)
    idx = sf['idx']
    pt = RL.point_records(sf['pts'], -rd[idx], sf['normal'], RL.estimator_materials(sf['mat5']), *RL.pixel_rotations(idx, 0))
    tab = RL.sample_table(32, 'cuda')
    mesh = (rl.verts, rl.tris.int(), rl.mat5, None)
    key = RL.pixel_keys(idx, 0)
    got = RL.relight_points(rl.tracer, pt, tab, tab, rl.env, 2, bounces=1, mesh=mesh, key=key)
    base = RL.relight_points(rl.tracer, pt, tab, tab, rl.env, 2)
    state = RL.relight_bounce_rays(rl.tracer, pt, tab, tab, mesh, key)['state'].reshape(len(idx), -1)
    free = (state < 2).all(-1)
    print(f'convex mesh: {int(free.sum())} of {len(idx)} points have no lane that meets the mesh ({float((state >= 2).float().mean()):.2%} of all lanes graze a facet)')
    assert int(free.sum()) > 0.5 * len(idx) and not got[3][free].any() and torch.equal(_bits(got[0][free]), _bits(base[0][free]))
    assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]) and float(got[3].min()) >= 0


# ---- a face that names a vertex the mesh does not have ----------------------------------------------------------------------------------------
def test_a_bad_face_index_contributes_nothing_and_reads_nothing(RL, tracers):
    """one face of a tris copy names vertex index V; verts, mat5 (and normals) are allocated with one spare row, so even an unchecked read
    would stay inside the allocation.  Lanes that hit that face report state 4 and contribute 0; every other lane is as before."""
    tr = tracers['corner']
    s = _device_case(RL, tr, 5, 65, 33, 32, 0, 'corner')
    V, Fc, vm, _ = s['mesh_dev']
    nV = V.shape[0]
    spare = lambda t: torch.cat([t, torch.full_like(t[:1], 1e3)]).contiguous()[:nV]           # a view of nV rows over nV + 1 allocated
    bad = Fc.clone()
    bad[2, 1] = nV
    good_mesh, bad_mesh = (spare(V), Fc, spare(vm), None), (spare(V), bad, spare(vm), None)
    tabs = (s['tab_d'].cuda(), s['tab_s'].cuda())
    run = lambda m: RL.relight_points(tr, s['pt'], *tabs, s['env'].cuda(), s['conv'], s['rot'], s['clamp'], 0, bounces=1, mesh=m, key=s['key_dev'])
    g, b = run(good_mesh), run(bad_mesh)
    rg = RL.relight_bounce_rays(tr, s['pt'], *tabs, good_mesh, s['key_dev'])
    rb = RL.relight_bounce_rays(tr, s['pt'], *tabs, bad_mesh, s['key_dev'])
    hit = rg['face'] == 2
    assert int(hit.sum()) > 20 and bool((rb['state'][hit] == 4).all()) and torch.equal(rb['state'][~hit], rg['state'][~hit])
    assert torch.equal(rb['face'], rg['face']) and not rb['sec_d'][hit].any() and bool((rb['strategy'][hit] == -1).all())
    touched = hit.reshape(65, -1).any(-1)
    assert torch.equal(_bits(g[3][~touched]), _bits(b[3][~touched])) and torch.equal(g[1], b[1]) and torch.equal(g[2], b[2])
    assert bool((b[3][touched] <= g[3][touched]).all()) and bool((b[3][touched] < g[3][touched]).any()) and bool(torch.isfinite(b[0]).all())


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def _corner_relighter(RL, tracers):
    V, Fc, _ = B.corner_scene()
    vm = B.vertex_materials(len(V), 9)
    mats = {'metallic': vm[:, 0:1].numpy(), 'roughness': vm[:, 1:2].numpy(), 'albedo': vm[:, 2:5].numpy()}
    Rm = torch.as_tensor(np.asarray(RR.ROT, np.float64))
    centre = (torch.tensor([[0.35, 0.35, 0.35]], dtype=F64) @ Rm.T)[0]
    rl = RL.Relighter(V, Fc, mats, RR.proper_map(16, 32, seed=2), convention='blender', tracer=tracers['corner'])
    # a camera inside the octant the corner encloses, looking at the corner: the orbit pose about the centre of the three quads
    eye = centre + (torch.tensor([1.0, 1.0, 1.0], dtype=F64) @ Rm.T) * 1.1
    z = torch.nn.functional.normalize(centre - eye, dim=0)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=F64) @ Rm.T
    x = torch.nn.functional.normalize(torch.linalg.cross(z, up), dim=0)
    y = torch.linalg.cross(z, x)
    Rw = torch.stack([x, y, z])
    pose = torch.cat([Rw, (-Rw @ eye)[:, None]], -1).numpy()
    return rl, pose, vm


def test_render_with_one_bounce(RL, tracers):
    """Relighter.render(bounces=1) for 12 pixels of the corner against the restatement from the camera ray on (brute-force hits, interpolation,
    record, rays, both walks, lookup, estimator); bounces=0 is the call without the argument in every key; bounces=2 is refused"""
    rl, pose, vm = _corner_relighter(RL, tracers)
    h = w = 48
    Dd = Ds = 32
    out = rl.render(pose, KMAT, h, w, samples=(Dd, Ds), seed=5, bounces=1)
    plain, zero = rl.render(pose, KMAT, h, w, samples=(Dd, Ds), seed=5), rl.render(pose, KMAT, h, w, samples=(Dd, Ds), seed=5, bounces=0)
    assert set(zero) == set(plain) and 'indirect_lin' not in plain and set(out) == set(plain) | {'indirect_lin'}
    for k in plain:
        assert torch.equal(zero[k], plain[k]), k
    for k in ('alpha', 'depth', 'albedo', 'metallic', 'roughness', 'normal'):
        assert torch.equal(out[k], plain[k]), k
    hit = out['alpha'][..., 0] > 0
    assert int(hit.sum()) > 300 and tuple(out['indirect_lin'].shape) == (h, w, 3) and float(out['indirect_lin'].min()) >= 0
    assert bool(torch.isfinite(out['rgb_lin']).all()) and float(out['indirect_lin'][hit].mean()) > 0.02 * float(out['rgb_lin'][hit].mean())
    assert bool((out['rgb_lin'][hit] >= plain['rgb_lin'][hit]).all()) and not out['indirect_lin'][~hit].any()
    two = rl.render(pose, KMAT, 24, 24, samples=(8, 8), ssaa=2, bounces=1)
    assert tuple(two['indirect_lin'].shape) == (24, 24, 3) and bool(torch.isfinite(two['indirect_lin']).all())
    with pytest.raises(ValueError, match='bounces'):
        rl.render(pose, KMAT, 8, 8, bounces=2)
    V, Fc = rl.verts.cpu(), rl.tris.cpu()
    tab = RR.sample_table(32)
    ref, picked = {}, None
    for dt in (F64, F32):
        o, d = RR.camera_rays(pose, KMAT, h, w, dt)
        depth, face, bary, margin = RR.closest_hit(V.to(dt), Fc, o, d)
        if picked is None:
            cand = torch.nonzero((face >= 0) & (margin > 1e-3))[:, 0]
            picked = cand[torch.linspace(0, len(cand) - 1, 12).long()]
        f, b = face[picked], bary[picked]
        corner = V.to(dt)[Fc[f]]
        n = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
        n = torch.where((n * d[picked]).sum(-1, keepdim=True) > 0, -n, n)
        mat5 = RR.interpolate(vm.to(dt), Fc, f, b)
        mat5 = torch.cat([mat5[:, :1], mat5[:, 1:2] ** 2, mat5[:, 2:]], -1)
        rd_, rs_ = RL.pixel_rotations(picked, 5)
        pt, dec_p = R.point_setup(RR.interpolate(V.to(dt), Fc, f, b), -d[picked], n, mat5, rd_.to(dt), rs_.to(dt))
        wd, od, dead, _ = B.primary_rays(pt, tab, tab, None, None, None, 0)
        key = RL.pixel_keys(picked, 5).numpy()
        m = (V, Fc, vm, None)
        state, fc2, bary2, blocked2, dec_f = B.facts(pt, wd, od, dead, None, key, m, Dd, Ds, 0, 0)
        res = B.bounce(pt, wd, None, state, fc2, bary2, blocked2, key, m, rl.env.cpu(), 2, None, 0.0, Dd, Ds, 0, 0)
        dec = {**res['dec'], **dec_f, 'dead_margin': R.dead_rays(pt, wd, Dd, Ds, 0)[1]['dead_margin']}
        ref[dt] = (res, B.exempt(dec), torch.minimum(dec_p['ortho_n'][1], dec_p['ortho_r'][1]))
    ok = ~ref[F64][1] & (ref[F64][2] > 1e-3)                                           # no grazing walk, no tie in a frame's choice
    floor = err = 0.0
    for k, name in (('rgb', 'rgb_lin'), ('indirect', 'indirect_lin')):
        got = out[name].reshape(-1, 3)[picked.cuda()].cpu()
        f_, e_ = RR.floors_and_errors(got, ref[F32][0][k], ref[F64][0][k], float(rl.env.mean()))
        floor, err = max(floor, float(f_[ok].max())), max(err, float(e_[ok].max()))
    floor = max(floor, ULP)
    share = float((ref[F64][0]['indirect'][ok] / ref[F64][0]['rgb'][ok]).mean())
    print(f'render with one bounce: {int(ok.sum())} of {len(picked)} pixels compared, indirect / rgb = {share:.2f} there; floor {floor:.2e} kernel {err:.2e} '
          f'({err / floor:.2f} floors)')
    assert int(ok.sum()) >= 6 and err <= K * floor


def test_the_script_takes_bounces(RL, tmp_path):
    from nero_amd.envlight import write_hdr
    from nero_amd.mesh import write_ply
    from nero_amd.texture import read_png
    V, Fc = RR.scene()
    write_ply(str(tmp_path / 'm.ply'), V.numpy(), Fc.numpy())
    vm = B.vertex_materials(len(V), 2)
    mats = {'metallic': vm[:, 0:1].numpy(), 'roughness': vm[:, 1:2].numpy(), 'albedo': vm[:, 2:5].numpy()}
    os.makedirs(tmp_path / 'mat')
    for k, a in mats.items():
        np.save(tmp_path / 'mat' / f'{k}.npy', a)
    write_hdr(str(tmp_path / 'e.hdr'), RR.proper_map(8, 16, seed=6).numpy())
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'relight.py'), '--mesh', str(tmp_path / 'm.ply'), '--material', str(tmp_path / 'mat'),
           '--hdr', str(tmp_path / 'e.hdr'), '--name', 'orbit', '--out', str(tmp_path / 'out'), '--num', '2', '--width', '32', '--height', '32',
           '--samples', '16', '16', '--cam_dist', '2.0', '--elevation', '70', '--bounces', '1']
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert '1 bounces' in run.stdout and sorted(os.listdir(tmp_path / 'out' / 'orbit')) == ['0.png', '1.png']
    rl = RL.Relighter(V, Fc, mats, str(tmp_path / 'e.hdr'))
    poses = RL.poses_in_mesh_frame(RL.relighting_poses(2, 0.0, 70.0, 2.0))
    for k in range(2):
        img = read_png(str(tmp_path / 'out' / 'orbit' / f'{k}.png'))
        want = rl.render(poses[k], RL.default_K(32, 32), 32, 32, samples=(16, 16), bounces=1)['rgba8'].cpu().numpy()
        assert img.shape == (32, 32, 4) and 50 < int((img[..., 3] > 0).sum()) < 1000 and np.array_equal(img, want)
        direct = rl.render(poses[k], RL.default_K(32, 32), 32, 32, samples=(16, 16))['rgba8'].cpu().numpy()
        assert np.array_equal(img[..., 3], direct[..., 3]) and not np.array_equal(img, direct)
    bad = subprocess.run(cmd[:-1] + ['2'], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and 'bounces' in bad.stderr


# ---- the width of a wavefront's partial -------------------------------------------------------------------------------------------------------
GUARD = 256


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('bounces', [0, 1])
@pytest.mark.parametrize('Dd,Ds,Dl', [(3, 2, 0), (33, 32, 0), (16, 16, 32), (33, 32, 7)])
def test_a_fused_call_writes_all_of_its_workspace_and_nothing_beyond(RL, L, tracers, Dd, Ds, Dl, bounces, mode):
    """each of the four fused entry points through the C ABI, on both walks, with a workspace of exactly the bytes its sizer states, cut
    from the middle of a buffer of 0xFF bytes (an unwritten partial reads as NaN): the 256 bytes on either side stay 0xFF, every output is
    finite, and every output has the bits of the same call with four times the workspace.  One padded wavefront per point, two with the
    second nearly empty, exactly one full, and two under the MIS estimator -- six floats per wavefront, twelve with the bounce."""
    P_, lib = 3, L.lib
    tr = tracers['corner']
    s = _device_case(RL, tr, 7, P_, Dd, Ds, Dl, 'corner')
    mis = Dl > 0
    counts = (Dd, Ds, Dl) if mis else (Dd, Ds)
    fused, sizer = {(False, 0): (lib.nero_bvh_relight, lib.nero_relight_workspace_bytes),
                    (True, 0): (lib.nero_bvh_relight_mis, lib.nero_relight_mis_workspace_bytes),
                    (False, 1): (lib.nero_bvh_relight_bounce, lib.nero_relight_bounce_workspace_bytes),
                    (True, 1): (lib.nero_bvh_relight_mis_bounce, lib.nero_relight_mis_bounce_workspace_bytes)}[mis, bounces]
    need = int(sizer(P_, *counts))
    assert need == P_ * ((Dd + Ds + Dl + 63) // 64) * (12 if bounces else 6) * 4
    tab_d, tab_s, env = s['tab_d'].cuda(), s['tab_s'].cuda(), s['env'].cuda().float().contiguous()
    light = (L.ptr(s['mis']['tab_l']), L.ptr(s['mis']['rand_l'].float().contiguous())) if mis else ()
    env_args = (L.ptr(env), env.shape[0], env.shape[1], int(RL.CONVENTIONS.get(s['conv'], s['conv'])), RL._rot_arg(s['rot']), float(s['clamp'] or 0.0))
    if mis:
        env_args += (L.ptr(s['table'].cdf), L.ptr(s['table'].info))
    V, Fc, vm, nrm = s['mesh_dev']
    key = RL._key_arg(s['key_dev'], P_, V.device)
    scene = (L.ptr(V), V.shape[0], L.ptr(Fc), Fc.shape[0], L.ptr(vm), L.ptr(nrm), L.ptr(key)) if bounces else ()

    def call(ws):
        out = [torch.full((P_, 3), float('nan'), device='cuda') for _ in range(4 if bounces else 3)]
        L.check(fused(tr._handle(), L.ptr(s['pt']), L.ptr(tab_d), L.ptr(tab_s), *light, P_, *counts, 0, *env_args, *scene, *[L.ptr(o) for o in out],
                      L.ptr(ws), ws.numel(), L.stream_ptr()))
        torch.cuda.synchronize()
        return out

    L.check(lib.nero_bvh_set_traversal(tr._handle(), mode))
    try:
        buf = torch.full((GUARD + need + GUARD,), 0xFF, dtype=torch.uint8, device='cuda')
        got = call(buf[GUARD:GUARD + need])
        roomy = call(torch.full((4 * need,), 0xFF, dtype=torch.uint8, device='cuda'))
    finally:
        L.check(lib.nero_bvh_set_traversal(tr._handle(), 1))
    assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + need:] == 0xFF).all())
    for k, (a, b) in enumerate(zip(got, roomy)):
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(_bits(a), _bits(b)), k
