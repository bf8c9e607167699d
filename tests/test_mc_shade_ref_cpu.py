"""CPU tier: pins tests/mc_shade_ref.py -- the reference tests/test_mc_shade_kernels_gpu.py compares the Stage-II shading and loss kernels
with -- without a GPU: (a) composed in shade_mixed order on golden Stage-II cases, with the oracle's own MLP outputs captured and fed in as
the raw heads, it reproduces the oracle in float64 to rounding: light-MLP inputs, outputs, losses and the gradients with respect to the
materials and the raw heads; (b) its autograd passes gradcheck; (c) the edge input sets of the GPU tier populate every branch side and
keep every row clear of every DERIVED boundary by the stated margin, with the float32 evaluation taking the float64 decisions; (d) the
float32 floors per condition class are measured, and the regular class meets 1e-4 on every forward output; (e) each of the named wrong
variants of the reference is rejected by the judge of the GPU tier, with its bounds, on a committed input set."""
import pytest
import torch

from oracle import nero_oracle as O
from oracle import nero_oracle_mat as M
from tests import mc_shade_ref as R
from tests import test_mc_shade_kernels_gpu as G
from tests.helpers import T as TT
from tests.helpers import build_material_case, load_golden, oracle_trace_fn, parity_report

F32, F64 = torch.float32, torch.float64


def _close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) <= tol


# ---- (a) against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mat_bell', 'mat_bear', 'mat_bell_smith'])          # plain; human light + sphere_direction; ggx_smith
def test_reference_composes_to_the_oracle(name, monkeypatch):
    z, meta = load_golden(name)
    net = build_material_case(meta).double()
    sd = {k: v for k, v in net.named_parameters()}
    sd.update({k: v for k, v in net.named_buffers()})
    Pm = O.effective_params(sd)
    scfg = {**M.DEFAULT_SHADER_CFG, **meta['shader_cfg']}
    rec = {'pred': [], 'trace': None}
    o_pred = M.predictor

    def pred(P_, prefix, x, out_act):
        raw = o_pred(P_, prefix, x, lambda t: t)
        rec['pred'].append((prefix.split('.')[-1], x, raw))
        return out_act(raw)
    monkeypatch.setattr(M, 'predictor', pred)
    tr = oracle_trace_fn()

    def trace(o, d):
        out = tuple(t.double() if t.is_floating_point() else t for t in tr(o.float(), d.float()))
        rec['trace'] = (o, d) + out
        return out
    c = lambda k: TT(z, k).double()
    pts, view, normals, poses, gt = c('pts'), c('view'), c('normals'), c('human_poses'), c('gt')
    out = M.material_train_outputs(Pm, {'shader_cfg': meta['shader_cfg']}, trace, pts, view, normals, poses, gt, meta['step'], c('rand_d'),
                                   c('rand_s'), c('reg_ang'), c('reg_eps'))
    total = M.material_training_loss(out)
    human, sphere = bool(scfg['human_lights']), scfg['outer_light_version'] == 'sphere_direction'
    geom = {'schlick': 0, 'ggx_smith': 1}[scfg['geometry_type']]
    preds = rec['pred']
    mats = ['metallic_predictor', 'roughness_predictor', 'albedo_predictor']
    assert [p[0] for p in preds] == mats + ['outer_light'] + (['human_light'] if human else []) + ['inner_light'] + mats
    raw, xin = (lambda i: preds[i][2]), (lambda i: preds[i][1])
    ki = 5 if human else 4
    # ---- forward, in shade_mixed order
    P_, Dd, Ds = pts.shape[0], scfg['diffuse_sample_num'], scfg['specular_sample_num']
    D = Dd + Ds
    mat5 = R.mat_head(torch.cat([raw(0), raw(1), raw(2)], -1))
    assert _close(mat5, torch.cat([out['metallic'], out['roughness'], out['albedo']], -1))
    pt, _ = R.point_setup(pts, view, normals, mat5, c('rand_d')[:, 0, 0], c('rand_s')[:, 0, 0])
    tab_d, tab_s = R._tab(Dd).double(), R._tab(Ds).double()
    w, orig = R.dirs(pt, tab_d, tab_s)
    t_o, t_d, inters, nrm, depth, hit = rec['trace']
    assert _close(w, t_d) and _close(orig, t_o)
    depth = depth[:, 0]
    dead = R.dead_rays(pt, w, Dd, Ds, geom)[0]
    hum = R.human_flags(pt, w, poses, D)[0] if human else None
    slot, miss_idx, hit_idx, n_hum = R.split(depth, dead, hum)
    assert int(dead.sum()) > 0 or geom == 1
    # rows of the oracle's miss / hit lists (ray order, dead rays included) that ours (partitioned, dead rays dropped) correspond to
    row_of = torch.zeros(P_ * D, dtype=torch.long)
    row_of[torch.nonzero(~hit)[:, 0]] = torch.arange(int((~hit).sum()))
    row_of[torch.nonzero(hit)[:, 0]] = torch.arange(int(hit.sum()))
    mo, ho = row_of[miss_idx.long()], row_of[hit_idx.long()]
    assert bool((~hit[miss_idx.long()]).all()) and bool(hit[hit_idx.long()].all())
    X_miss = R.encode_miss(w, miss_idx, pt, D, sphere)
    X_hit = R.encode_hit(w, inters, -nrm, hit_idx)
    assert X_miss.shape[1] == (144 if sphere else 72) and _close(X_miss, xin(3)[mo]) and _close(X_hit[:, :123], xin(ki)[ho])
    assert float(X_hit[:, 123:].abs().max()) == 0
    human_raw = hmask = None
    if human:
        Xh, hmask = R.human_encode(w, miss_idx[:n_hum], pt, D, poses)
        assert 0 < n_hum < miss_idx.numel() and _close(Xh, xin(4)[mo[:n_hum]]) and bool((hmask == 1).all())
        human_raw = raw(4)[mo[:n_hum]]
    emax, imax = scfg['light_exp_max'], scfg['inner_light_exp_max']
    rgb_lin, dl, sl, spec, _ = R.combine_fwd(pt, w, depth, slot, raw(3)[mo], raw(ki)[ho], human_raw, hmask, n_hum, emax, imax, Dd, Ds, geom)
    srgb01 = lambda t: torch.clamp(O.linear_to_srgb(t), 0, 1)
    assert _close(O.linear_to_srgb(rgb_lin), out['rgb_pr']) and _close(srgb01(dl), out['diffuse_light'])
    assert _close(srgb01(sl), out['specular_light']) and _close(srgb01(spec), out['specular_color'])
    # ---- the loss glue
    reg_pts = R.reg_points(pts, normals, c('reg_ang')[:, 0], c('reg_eps')[:, 0])
    assert _close(reg_pts[P_:], xin(ki + 1)[:, -3:]) and torch.equal(reg_pts[:P_], pts)
    mat = torch.cat([mat5, R.mat_head(torch.cat([raw(ki + 1), raw(ki + 2), raw(ki + 3)], -1))])
    cfg = dict(rgb_l1=0, reg_mat=1, reg_change=int(scfg['reg_change']), reg_lambda1=scfg['reg_lambda1'],
               hinge_weight=1.0 if scfg['reg_min_max'] and meta['step'] < 2000 else 0.0, reg_diffuse=1, reg_diffuse_lambda=0.1)
    loss, rgb_pr, _ = R.mat_loss(cfg, P_, 1, mat, rgb_lin, dl, gt)
    want = torch.stack([total, out['loss_rgb'].mean(), out['loss_mat_reg'].mean(), out['loss_diffuse_light'].mean()])
    assert _close(rgb_pr, out['rgb_pr'])
    for k in range(4):
        assert _close(loss[k], want[k]), k
    # ---- gradients: the oracle's autograd with respect to the materials, the raw heads and (the cotangents of ours) the light-MLP inputs
    wrt = [out['metallic'], out['roughness'], out['albedo'], raw(3), raw(ki), xin(3), xin(ki)] + ([raw(4), xin(4)] if human else [])
    g = torch.autograd.grad(total, wrt, allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for t, x in zip(wrt, g)]
    d_mat, d_rgb, d_dl = R.mat_loss_bwd(cfg, P_, 1, mat, rgb_lin, dl, gt)
    dX_hit = torch.zeros(hit_idx.numel(), 128, dtype=F64)
    dX_hit[:, :123] = g[6][ho]
    q = dict(P=P_, Dd=Dd, Ds=Ds, sphere=int(sphere), pt=pt.detach(), dirs=w.detach(), tab_s=tab_s, depth=depth, slot=slot, miss_idx=miss_idx,
             hit_idx=hit_idx, n_hum=n_hum if human else 0, outer_raw=raw(3)[mo].detach(), inner_raw=raw(ki)[ho].detach(),
             human_raw=None if not human else human_raw.detach(), hmask=hmask, emax=emax, imax=imax, pos=inters, fnrm=-nrm, poses=poses,
             d_rgb=d_rgb, d_dl=d_dl, dX_miss=g[5][mo], dX_hit=dX_hit, dXh=g[8][mo[:n_hum]] if human else None)
    b = R.shading_bwd(q, geom)
    assert _close(b['d_mat5'] + d_mat[:P_], torch.cat(g[:3], -1))
    assert _close(b['d_outer_raw'], g[3][mo]) and _close(b['d_inner_raw'], g[4][ho])
    gone = torch.ones(g[4].shape[0], dtype=torch.bool)
    gone[ho] = False
    assert float(g[4][gone].abs().max() if bool(gone.any()) else 0.0) == 0     # the dead rays' rows carry exactly nothing in the oracle
    if human:
        assert _close(b['d_human_raw'], g[7][mo[:n_hum]])
        rest = torch.ones(g[7].shape[0], dtype=torch.bool)
        rest[mo[:n_hum]] = False
        assert float(g[7][rest].abs().max()) == 0                             # rows the human-light MLP does not own: masked out


# ---- (b) autograd of the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', [0, 1])
def test_gradcheck_of_the_estimator_and_the_loss(geom):
    q = R.estimator_inputs(2, 3, 5, 1, 1)
    assert int(q['cls'].sum()) == 0 and q['n_hum'] > 0 and q['hit_idx'].numel() > 0 and q['miss_idx'].numel() > q['n_hum']
    d = lambda k: q[k].double()
    P_, Dd, Ds = 2, 3, 5
    mi, hi = q['miss_idx'].long(), q['hit_idx'].long()
    pm = R._pidx(mi, Dd + Ds)
    depth = torch.where(d('depth') < 10, d('depth').clamp(min=0.1), d('depth'))                      # rows clear of every clamp
    outer, inner = d('outer_raw').clamp(max=q['emax'] - 0.2), d('inner_raw').clamp(max=q['imax'] - 0.2)
    human, hmask = -0.1 - d('human_raw').abs(), (d('hmask') != 0).double()

    def fn(mat5, o_raw, i_raw, h_raw):
        pt = torch.cat([d('pt')[:, :9], mat5, d('pt')[:, 14:]], -1)
        w = torch.cat([d('dirs').reshape(P_, -1, 3)[:, :Dd], R.specular_dirs(pt, d('tab_s'))], 1)
        L, _ = R.lights(q['slot'], depth, o_raw, i_raw, h_raw, hmask, q['n_hum'], q['emax'], q['imax'])
        est = R.estimator(pt, mat5[:, None], w, L.reshape(P_, -1, 3), Dd, Ds, geom)[:4]
        wr = w.reshape(-1, 3)
        nh = q['n_hum']
        return est + (R.miss_rows(wr[mi], pt[pm, 29:32], 1), R.hit_rows(wr[hi], d('pos')[hi], d('fnrm')[hi])[:, 51:123],
                      R.human_rows(wr[mi[:nh]], pt[pm[:nh], 29:32], d('poses')[pm[:nh]])[0])
    xs = tuple(t.clone().requires_grad_(True) for t in (d('pt')[:, 9:14], outer, inner, human))
    assert torch.autograd.gradcheck(fn, xs, eps=1e-6, atol=1e-6, rtol=1e-5)
    g = R._gen(3)
    n = 6
    mat = 0.2 + 0.6 * torch.rand(2 * n, 5, generator=g, dtype=F64)
    mat[0, 1], mat[1, 1], mat[2, 0], mat[3, 0] = 0.99, 1e-4, 0.995, 0.01                           # inside all four hinges
    rgb, dl = 0.05 + torch.rand(n, 3, generator=g, dtype=F64), 0.05 + 0.5 * torch.rand(n, 3, generator=g, dtype=F64)
    rgb[0], dl[0] = 1e-3 * (1 + torch.arange(3, dtype=F64)), 1e-3 * (1 + torch.arange(3, dtype=F64))      # below the sRGB knee
    gt = torch.rand(n, 3, generator=g, dtype=F64)
    for cfg in R.LOSS_CFGS:
        xs = tuple(t.clone().requires_grad_(True) for t in (mat, rgb, dl))
        assert torch.autograd.gradcheck(lambda a, b_, c_: R.mat_loss(cfg, n, cfg['has_reg'], a, b_, c_, gt)[:2], xs, eps=1e-7, atol=1e-6, rtol=1e-5)
    raw = torch.randn(n, 5, generator=g, dtype=F64).requires_grad_(True)
    assert torch.autograd.gradcheck(R.mat_head, (raw,), eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- (c) the edge input sets of the GPU tier -------------------------------------------------------------------------------------------------
def _both(dec, key, approach, mask=None):
    side, dist = dec[key]
    if mask is not None:
        side, dist = side[mask], dist[mask]
    if key in R.MARGINS and dist.numel():
        approach[key] = min(approach.get(key, 1e30), float(dist.min()))
    return int(side.sum()), int((~side).sum())


def test_estimator_inputs_cover_every_branch_with_margin():
    """measured closest approaches over all committed estimator sets: recorded in parity_report by the GPU tier's shapes and printed here"""
    approach, sides, combos, clamp_rows = {}, {}, {}, {}
    for i in range(len(R.EST_CASES)):
        key = G._case_key(i)
        P_, Dd, Ds, human, sphere, _ = key
        q = R.estimator_inputs(*key)
        c = R.point_inputs(P_, Dd, Ds, q['seed'])
        combos.setdefault(P_, []).append((human, sphere))
        n_miss = q['miss_idx'].numel()
        assert (0 < q['n_hum'] < n_miss) if human else q['n_hum'] == 0, key       # the human-light MLP owns some, not all, miss rows
        d64, d32 = R.point_decisions(c, c['tab_d'], c['tab_s'], F64), R.point_decisions(c, c['tab_d'], c['tab_s'], F32)
        f = lambda k, dt: None if q[k] is None else q[k].to(dt)
        for dt, dec in ((F64, d64), (F32, d32)):
            dec.update(R.lights(q['slot'], f('depth', dt), f('outer_raw', dt), f('inner_raw', dt), f('human_raw', dt), f('hmask', dt), q['n_hum'],
                                q['emax'], q['imax'])[1])
        for k, (side, dist) in d64.items():
            keep = ~R._exempt(k, c) if side.shape[0] == P_ and k not in ('outer_cap', 'inner_cap', 'human_cap', 'hw_hi', 'hw_lo', 'near') else None
            if keep is not None:
                assert torch.equal(side[keep], d32[k][0][keep]), (key, k)    # float32 decides like float64
            else:
                assert torch.equal(side, d32[k][0]), (key, k)
            a, b = _both(d64, k, approach, keep)
            sides[k] = (sides.get(k, (0, 0))[0] + a, sides.get(k, (0, 0))[1] + b)
            if k in R.MARGINS and (keep is None or bool(keep.any())):
                dd = dist if keep is None else dist[keep]
                if k == 'hw_hi':                                             # exp(min(raw, 0)) x mask: exactly 1 when raw >= 0 (a tie, direct)
                    dd = dd[dd != 0]
                assert not dd.numel() or float(dd.min()) >= R.MARGINS[k], (key, k, float(dd.min()))
        if human and q['n_hum'] > 6:                                         # the rows that reach the clamp of the human weight from both sides
            assert bool((q['human_raw'] == 0).any()) and {0.0, 1.0, 2.0, -0.5} <= set(q['hmask'].tolist())
            clamp_rows[P_] = clamp_rows.get(P_, 0) + 1
        if P_ == 65:
            assert q['hit_idx'].numel() > 0 and int(q['dead'].sum()) > Dd + Ds
            assert set(q['kind'].tolist()) == set(range(-1, len(R.EXTREME_KINDS)))                  # every extreme kind, and regular points
            assert bool((q['depth'] == 1e-5).any()) and bool((q['depth'] == 10.0).any()) and bool((q['depth'] == 0).any())
            assert bool((q['outer_raw'][:, :3] == q['emax']).any()) and bool((q['inner_raw'][:, :3] == q['imax']).any())
    for P_ in R.EST_P:                                                       # every P meets every (human, sphere) setting
        assert set(combos[P_]) == {(0, 0), (0, 1), (1, 0), (1, 1)}, (P_, combos[P_])
    assert clamp_rows.get(65, 0) == 4 and clamp_rows.get(3, 0) >= 2, clamp_rows
    for k in ('nw', 'nH', 'dead_margin', 'ortho_n', 'ortho_r', 'nov0', 'dz_small', 'dist_pos', 'radius', 'pnorm', 'outer_cap', 'inner_cap', 'human_cap',
              'hw_hi', 'hw_lo', 'near'):
        assert min(sides[k]) > 0, (k, sides[k])
    print('closest approaches', approach)
    print('sides', sides)
    parity_report('mc_shade_ref::estimator_inputs', closest_approach=approach, margins={k: R.MARGINS[k] for k in approach}, sides={k: list(v) for k, v in sides.items()})


def test_loss_inputs_cover_every_branch_with_margin():
    approach = {}
    for P_ in R.LOSS_P:
        s = R.loss_inputs(P_)
        cfg = R.LOSS_CFGS[0]
        dec = {dt: R.mat_loss(cfg, P_, 1, s['mat'].to(dt), s['rgb_lin'].to(dt), s['dl'].to(dt), s['gt'].to(dt))[2] for dt in (F64, F32)}
        for k, (side, dist) in dec[F64].items():
            tie = dist == 0                                                  # exact ties are built from direct inputs (all-clamped / all-zero rows, dl == 1)
            assert torch.equal(side[~tie], dec[F32][k][0][~tie]), (P_, k)
            if bool((~tie).any()):
                approach[k] = min(approach.get(k, 1e30), float(dist[~tie].min()))
                assert float(dist[~tie].min()) >= R.MARGINS[k], (P_, k, float(dist[~tie].min()))
            if P_ >= 255:
                assert int(side.sum()) > 0 and int((~side).sum()) > 0, (P_, k)
        if P_ >= 255:
            m, r = s['mat'][:P_, 0], s['mat'][:P_, 1]
            th = torch.tensor([R.H_R_HI, R.H_R_LO, R.H_M_HI, R.H_M_LO], dtype=F64).float()
            for col, t in ((r, th[0]), (r, th[1]), (m, th[2]), (m, th[3])):   # within 1e-6 of each hinge threshold on either side, and far from it
                assert bool(((col > t) & (col < t * (1 + 1e-6))).any()) and bool(((col < t) & (col > t * (1 - 1e-6))).any())
                assert not bool((col == t).any()) and bool((col > t + 0.01).any())
            d = s['mat'][P_:] - s['mat'][:P_]
            assert bool((d == 0).any()) and bool((d > 0).any()) and bool((d < 0).any())
            assert int(dec[F64]['sign_dl'][1].eq(0).sum()) >= 6 and bool((s['dl'] == 1.0).any())
    print('closest approaches', approach)
    parity_report('mc_shade_ref::loss_inputs', closest_approach=approach, margins={k: R.MARGINS[k] for k in approach})


# ---- (d) condition classes --------------------------------------------------------------------------------------------------------------------
def test_condition_class_floors():
    """float32 floors per (output, geometry, class, fewer than 16 directions), worst row over the committed estimator sets: measured here on
    the CPU, never on the kernel; the table is in the docstring of tests/mc_shade_ref.py.  The regular class stays at or below the 1e-4
    the end-to-end tests grant on every forward output (measured: 3.6e-5 at most)."""
    floors = G.est_floors()
    for (name, geom, cls, few), v in sorted(floors.items()):
        print(f'{name:12s} geom={geom} class={cls} few={int(few)} floor={v:.2e}')
        if cls == 0 and name in G.EST_OUT:
            assert v <= 1e-4, (name, geom, few, v)                            # never looser than the end-to-end tests
    assert {k[2] for k in floors} == {0, 1} and {k[3] for k in floors} == {False, True}
    parity_report('mc_shade_ref::fp32_floors', **{f'{n}@geom{g_},class{c_},few{int(f_)}': v for (n, g_, c_, f_), v in floors.items()})


# ---- (e) it would notice -----------------------------------------------------------------------------------------------------------------------
def _estimator_rejects(wrong):
    """the first committed input set on which the REGULAR class alone rejects the variant (an extreme row may only add to that)"""
    floors = G.est_floors()
    for i in reversed(range(len(R.EST_CASES))):                              # the large sets first
        key = G._case_key(i)
        q = R.estimator_inputs(*key)
        for geom in (0, 1):
            d_dl = G.use_d_dl(i, geom)
            refs, got = G.est_refs(key, geom, d_dl), G.est_eval(q, geom, d_dl, F64, wrong)
            # (a variant that divides by zero on some rows is judged on its finite rows: the BOUND has to reject it, not the isfinite check)
            got = {k: torch.where(torch.isfinite(v), v, refs[k][0]) for k, v in got.items()}
            report = {}
            fails = [f for name in got for f in G.judge_classes(report, name, geom, got[name].float(), refs[name], floors,
                                                                G.few_directions(q['Dd'], q['Ds']), classes=(0,)) if f]
            if fails:
                return key, geom, fails[0]
    return None


def _correct_reference_passes():
    floors = G.est_floors()
    key = G._case_key(len(R.EST_CASES) - 1)
    q = R.estimator_inputs(*key)
    for geom in (0, 1):
        refs = G.est_refs(key, geom, G.use_d_dl(len(R.EST_CASES) - 1, geom))
        got = {k: v[0].float() for k, v in refs.items()}                     # the float64 reference rounded to float32: what a perfect kernel returns
        report = {}
        assert not [f for name in got for f in G.judge_classes(report, name, geom, got[name], refs[name], floors, G.few_directions(q['Dd'], q['Ds'])) if f]


ESTIMATOR_WRONG = [w for w in R.WRONG if w not in ('no_pull_in', 'hinge_mean', 'reg_albedo_weight_1')]


def test_the_judge_accepts_the_reference_itself():
    _correct_reference_passes()


@pytest.mark.parametrize('wrong', ESTIMATOR_WRONG)
def test_wrong_estimator_variants_are_rejected(wrong):
    hit = _estimator_rejects(wrong)
    assert hit is not None, f'{wrong}: accepted on every committed input set -- the bound is too loose'
    print(wrong, 'rejected on', hit)


def test_wrong_pull_in_is_rejected_by_the_encoder_judge():
    hits = []
    for n, dd_ds in G.ENC_SHAPES:
        refs, bad = G.enc_refs(n, dd_ds), G.enc_refs(n, dd_ds, 'no_pull_in')
        report = {}
        hits += [f for f in G.judge_encoders(report, {k: bad[k][F64].float() for k in refs if k != 'hmask'}, refs) if f]
        assert not [f for f in G.judge_encoders({}, {k: refs[k][F64].float() for k in refs if k != 'hmask'}, refs) if f]
    assert hits and all(h[0] == 'X_miss@sphere1' for h in hits), hits


@pytest.mark.parametrize('wrong', ['hinge_mean', 'reg_albedo_weight_1'])
def test_wrong_loss_variants_are_rejected(wrong):
    hits = []
    for P_ in R.LOSS_P[1:]:
        for ci, cfg in enumerate(R.LOSS_CFGS):
            s, hr = R.loss_inputs(P_), cfg['has_reg']
            mat = (s['mat'] if hr else s['mat'][:P_]).double()
            scale = G.loss_grad_scale(ci)
            refs = G.loss_refs(P_, ci, scale)
            ls = [R.leaf(t, F64) for t in (mat, s['rgb_lin'], s['dl'])]
            loss, pr, _ = R.mat_loss(cfg, P_, hr, ls[0], ls[1], ls[2], s['gt'].double(), wrong)
            g = torch.autograd.grad(loss[0] * scale, ls, allow_unused=True)
            g = [torch.zeros_like(l) if x is None else x for l, x in zip(ls, g)]
            gots = dict(loss=loss.detach().float(), rgb_pr=pr.detach().float(), d_mat=g[0].float(), d_rgb_lin=g[1].float(), d_dl=g[2].float())
            hits += [(P_, ci, f[0]) for f in G.judge_loss({}, gots, refs) if f]
            good = {k: v[0].float() for k, v in refs.items()}
            assert not [f for f in G.judge_loss({}, good, refs) if f]
    assert hits, f'{wrong}: accepted on every committed input set -- the bound is too loose'
    assert {h[2] for h in hits} >= {'loss', 'd_mat'}, hits
