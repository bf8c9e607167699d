"""CPU tier: pins tests/shade_ref.py -- the reference tests/test_shade_kernels_gpu.py compares the shading / compositing kernels with --
without a GPU: (1) composed in the order of render_core / app_shading on golden Stage-I cases, with the oracle's own MLP outputs captured
and fed in as the raw heads, it reproduces the oracle in float64 to rounding; (2) its autograd passes gradcheck; (3) the edge input sets
the GPU tier uses populate every branch side and keep every row clear of every DERIVED boundary by the stated margin, with the float32
evaluation taking the float64 decisions."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nero_oracle as O
from tests import shade_ref as S
from tests.helpers import T as TT
from tests.helpers import build_case_model, load_golden, ref_fg_lut

F64 = torch.float64
PER_SAMPLE, COMPOSITE_WAVE_T, COMPOSITE_THREAD_T = S.PER_SAMPLE, S.COMPOSITE_WAVE_T, S.COMPOSITE_THREAD_T
ANNEALS = (0.0, 0.3, 1.0)


def _close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30)) <= tol


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['bell_s25000', 'bear_s25000', 'bell_sphdir'])       # plain; human light; sphere_direction
def test_reference_composes_to_the_oracle(name, monkeypatch):
    z, meta = load_golden(name)
    net = build_case_model(meta)
    P = O.effective_params({k: (v.detach().double() if v.is_floating_point() else v.detach()) for k, v in net.state_dict().items()})
    cfg = {**O.DEFAULT_CFG, **meta['cfg'], 'apply_occ_loss': False}
    scfg = cfg['shader_config']
    rec = {'pred': [], 'app': None, 'nerf': None, 'sdf': None}
    o_pred, o_nerf, o_sdf, o_app = O.predictor, O.nerfpp, O.sdf_value_and_normal, O.app_shading

    def pred(P_, prefix, x, out_act):
        raw = o_pred(P_, prefix, x, lambda t: t)
        rec['pred'].append((prefix.split('.')[-1], x, raw))
        return out_act(raw)

    def keep(key, fn):
        def f(*a, **k):
            rec[key] = fn(*a, **k)
            return rec[key]
        return f
    monkeypatch.setattr(O, 'predictor', pred)
    monkeypatch.setattr(O, 'nerfpp', keep('nerf', o_nerf))
    monkeypatch.setattr(O, 'sdf_value_and_normal', keep('sdf', o_sdf))
    monkeypatch.setattr(O, 'app_shading', keep('app', o_app))
    c = lambda k: TT(z, k).double()
    o, d, zv, poses = c('o'), c('d'), c('z_vals'), c('human_poses')
    with torch.no_grad():
        out = O.render_core(P, cfg, o, d, zv, poses, meta['anneal'], meta['step'])
    R, T = zv.shape
    dists = torch.cat([zv[:, 1:] - zv[:, :-1], zv[:, -1:] - zv[:, -2:-1]], -1)
    pts = (o[:, None] + d[:, None] * (zv + dists * 0.5)[..., None]).reshape(-1, 3)
    inner = torch.norm(pts, dim=-1) <= 1.0
    ii, oi = torch.nonzero(inner)[:, 0], torch.nonzero(~inner)[:, 0]
    assert ii.numel() > 0 and oi.numel() > 0
    dflat = dists.reshape(-1)
    y, grad = rec['sdf']
    n = ii.numel()
    inv_s = S.inv_s_of(P['deviation_network.variance'], F64).reshape(1).expand(n)
    alpha_i, geo, gerr, _ = S.sdf_alpha(y[:, 0], grad, dflat[ii], d, S.ray_of(ii, T), inv_s, meta['anneal'])
    preds = rec['pred']
    names = [p[0] for p in preds]
    human = bool(scfg.get('human_light', False))
    assert names == ['metallic_predictor', 'roughness_predictor', 'albedo_predictor', 'outer_light', 'outer_light'] + \
        (['human_light_predictor'] if human else []) + ['inner_light', 'inner_weight']
    raw = lambda i: preds[i][2]
    mat = S.materials(raw(0), raw(1), raw(2))
    sphere = bool(scfg.get('sphere_direction', False))
    pi = pts[ii]
    Xd, Xs, Xi, Xo, _ = S.shade_encode(pi, geo[:, :3], geo[:, 4:7], mat[:, 1:2], sphere)
    k = 6 if human else 5
    for got, (_, want, _) in ((Xd, preds[3]), (Xs, preds[4]), (Xi[:, :123], preds[k]), (Xo[:, :90], preds[k + 1])):
        assert got.shape == want.shape and _close(got, want)
    assert Xd.shape[1] == (144 if sphere else 72) and float(Xi[:, 123:].abs().max()) == 0 and float(Xo[:, 90:].abs().max()) == 0
    Lh = hmask = None
    if human:
        Xh, hmask, _ = S.human_encode(pi, geo[:, 4:7], mat[:, 1:2], poses[S.ray_of(ii, T)])
        assert _close(Xh, preds[5][1]) and 0 < int(hmask.sum()) < n
        Lh = raw(5)
    color_i, occ, _ = S.combine_fwd(geo[:, 3], mat, raw(3), raw(4), raw(k), raw(k + 1), P['color_network.FG_LUT'], scfg.get('light_exp_max', 0.0),
                                    Lh, hmask)
    assert _close(color_i, rec['app'][0]) and _close(occ, rec['app'][1]['occ_prob'][:, 0]) and _close(geo[:, 4:7], rec['app'][1]['reflective'])
    sigma, rgb = rec['nerf']
    a_o, c_o, _ = S.nerf_head(sigma[:, 0], rgb, dflat[oi])
    aRT, cRT = S.scatter(alpha_i, color_i, ii, R * T, 0.0)
    aRT2, cRT2 = S.scatter(a_o, c_o, oi, R * T, 0.0)
    w, ray_rgb, _ = S.composite((aRT + aRT2).reshape(R, T), (cRT + cRT2).reshape(R, T, 3))
    assert _close(w, out['weights']) and _close(ray_rgb, out['ray_rgb']) and _close(gerr, out['gradient_error'])
    # the validation intermediates too (want_inter): the same captured heads through inter_results
    with torch.no_grad():
        rec['pred'].clear()
        _, _, inter = o_app(P, scfg, pi, grad, -F.normalize(d, dim=-1)[S.ray_of(ii, T)], y[:, 1:], poses[S.ray_of(ii, T)], want_inter=True)
    got = S.inter_results(geo[:, 3], mat, raw(3), raw(4), raw(k), raw(k + 1), P['color_network.FG_LUT'], scfg.get('light_exp_max', 0.0), Lh, hmask)
    cols = dict(specular_albedo=0, specular_ref=3, specular_light=6, specular_color=9, diffuse_albedo=12, diffuse_light=15, diffuse_color=18,
                metallic=21, roughness=22, occ_prob=23, indirect_light=24, human_light=27)
    for key, v in inter.items():
        assert _close(got[:, cols[key]:cols[key] + v.shape[1]], v), key


# ---- 2. autograd of the reference ----------------------------------------------------------------------------------------------------
def _gc(fn, *xs):
    assert torch.autograd.gradcheck(fn, tuple(x.double().clone().requires_grad_(True) for x in xs), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradcheck_of_every_reference():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    n, ray = 5, torch.tensor([0, 0, 1, 2, 2])
    d, dist = r(3, 3), 0.05 + torch.rand(n, generator=g, dtype=F64) * 0.1
    _gc(lambda sdf, grad, s: S.sdf_alpha(sdf, grad, dist, d, ray, s, 0.3)[:3], 0.02 * r(n), r(n, 3), 20 + r(n).abs())
    p = 0.5 * r(n, 3)
    p[0] = F.normalize(p[0], dim=-1) * 1.05                         # one row outside the 0.999 sphere
    for sphere in (False, True):
        _gc(lambda nh, rf, ro: S.shade_encode(p, nh, rf, ro, sphere)[:4], F.normalize(r(n, 3), dim=-1), F.normalize(r(n, 3), dim=-1),
            torch.rand(n, 1, generator=g, dtype=F64))
    _gc(lambda a, b, c: S.materials(a, b, c), r(n, 4), r(n, 4), r(n, 4))
    poses = torch.eye(3, 4, dtype=F64).expand(n, 3, 4).clone()
    poses[:, 2, 3] = 0.8
    rf = F.normalize(r(n, 3) * torch.tensor([1.0, 1.0, 0.0], dtype=F64) + torch.tensor([0.0, 0.0, -1.0], dtype=F64), dim=-1)
    Xh, hm, _ = S.human_encode(p, rf, torch.full((n, 1), 0.3, dtype=F64), poses)
    assert int(hm.sum()) >= 3
    _gc(lambda a, b: S.human_encode(p, a, b, poses)[0], rf, 0.2 + 0.5 * torch.rand(n, 1, generator=g, dtype=F64))
    lut = ref_fg_lut()
    mat = 0.2 + 0.6 * torch.rand(n, 5, generator=g, dtype=F64)
    nov = (torch.arange(n, dtype=F64) + 20.3) / 256                 # mid-texel: the LUT fetch is smooth there
    mat[:, 1] = (torch.arange(n, dtype=F64) + 100.7) / 256
    hmask = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], dtype=F64)
    for Lh in (None, -0.5 - r(n, 4).abs()):
        args = [nov, mat, -0.3 - r(n, 4).abs(), -0.3 - r(n, 4).abs(), -0.3 - r(n, 4).abs(), 0.5 * r(n, 4)] + ([Lh] if Lh is not None else [])
        _gc(lambda *a: S.combine_fwd(*a[:6], lut, 0.5, a[6] if len(a) > 6 else None, hmask if len(a) > 6 else None)[:2], *args)
    _gc(lambda s, c: S.nerf_head(s, c, dist)[:2], 3 * r(n), r(n, 3))
    _gc(lambda a, c: S.composite(a, c)[:2], torch.rand(3, 7, generator=g, dtype=F64) * 0.9, torch.rand(3, 7, 3, generator=g, dtype=F64))
    x, e, t = r(n, 3), r(n, 39), r(n, 3)
    assert _close(S.pe_vjp(x, e, 6), torch.einsum('nij,ni->nj', torch.stack([torch.autograd.functional.jacobian(lambda q: O.pos_enc(q, 6), x[i])
                                                                             for i in range(n)]), e))
    assert _close((S.pe_jvp(x, t, 6) * e).sum(), (S.pe_vjp(x, e, 6) * t).sum())          # <J t, e> == <t, J^T e>


# ---- 3. the edge input sets of the GPU tier ---------------------------------------------------------------------------------------------
def _sides(dec, key):
    s = dec[key][0]
    return int(s.sum()), int((~s).sum())


def _check(dec64, dec32, approach, skip=None):
    """margins of the derived boundaries, and the float32 evaluation deciding like the float64 one"""
    for key, (side, dist) in dec64.items():
        assert torch.equal(side, dec32[key][0]), key
        if key in S.MARGINS:
            dd = dist if skip is None or key not in skip else dist[~skip[key]]
            if dd.numel():
                approach[key] = min(approach.get(key, 1e30), float(dd.min()))
                assert float(dd.min()) >= S.MARGINS[key], (key, float(dd.min()))


def _alpha_dec(n, R, T, anneal, dt):
    a = S.alpha_inputs(n, R, T)
    c = lambda k: a[k].to(dt)
    return S.sdf_alpha(c('sdf4')[:, 0], c('grad'), c('x4')[:, 3], c('d'), a['ray'], S.inv_s_of(a['variance'], dt).expand(n), anneal)[3]


def test_alpha_inputs_cover_every_branch_with_margin():
    """measured closest approaches (all sets): relu_half 1.0e-2, relu_cos 2.0e-2, raw_lo 1.0e-5"""
    approach = {}
    for n, R, T in PER_SAMPLE:
        a = S.alpha_inputs(n, R, T)
        zero_row = a['grad'].abs().sum(-1) == 0                     # a DIRECT input: true_cos == 0 exactly in every precision
        assert a['idx'].shape == (n,) and int(a['idx'].max()) < R * T and bool((a['idx'][1:] >= a['idx'][:-1]).all())
        for an in ANNEALS:
            d64, d32 = _alpha_dec(n, R, T, an, F64), _alpha_dec(n, R, T, an, torch.float32)
            _check(d64, d32, approach, skip={'relu_cos': zero_row})
            if n >= 63:
                for key in ('relu_half', 'relu_cos', 'raw_lo', 'grad_zero'):
                    assert min(_sides(d64, key)) > 0, (n, key)
                assert int((d64['raw_hi'][1] == 0).sum()) > 0        # alpha saturated to exactly 1 (a tie: raw <= 1 always)
                assert len(set(a['ray'].tolist())) >= 2 and bool((a['x4'][:, 3] == 0).any())
                gn = torch.linalg.norm(a['grad'], dim=-1)
                assert float(gn.max()) > 1.5 and float(gn[gn > 0].min()) < 0.5
                assert float((torch.linalg.norm(a['d'], dim=-1) - 1).abs().min()) > 1e-3     # unnormalised ray directions
    print('closest approaches', approach)


def _shading_decs(n, R, T, dt, human=True):
    s = S.shading_inputs(n, R, T)
    c = lambda k: s[k].to(dt)
    dec = {}
    dec.update(S.shade_encode(c('p'), c('geo')[:, :3], c('geo')[:, 4:7], c('mat')[:, 1:2], True)[4])
    dec.update(S.human_encode(c('p'), c('geo')[:, 4:7], c('mat')[:, 1:2], c('poses')[s['ray']])[2])
    dec.update(S.combine_fwd(c('geo')[:, 3], c('mat'), c('Ld'), c('Ls'), c('Li'), c('Lo'), ref_fg_lut(), s['exp_max'],
                             c('Lh') if human else None, c('hmask') if human else None)[2])
    return dec


def test_shading_inputs_cover_every_branch_with_margin():
    """margins and measured closest approaches: stated next to the builders (tests/shade_ref.py::MARGINS)"""
    approach = {}
    both = ['sphere_pull', 'dz_small', 'dist_pos', 'radius', 'hit', 'exp_max_d', 'exp_max_s', 'exp_max_i', 'h_raw', 'hmask', 'occ_lo', 'occ_hi',
            'knee', 'out_hi', 'nov_lo', 'nov_hi', 'u_first', 'u_last', 'v_first', 'v_last']
    for n, R, T in PER_SAMPLE:
        s = S.shading_inputs(n, R, T)
        for human in (True, False):
            d64, d32 = _shading_decs(n, R, T, F64, human), _shading_decs(n, R, T, torch.float32, human)
            _check(d64, d32, approach)
            if n >= 63:
                for key in both:
                    if key in d64:
                        assert min(_sides(d64, key)) > 0, (n, human, key)
        if n >= 63:                                                  # direct inputs exactly ON their boundaries
            dh = _shading_decs(n, R, T, F64, True)
            # the blend weight exp(min(raw, 0)) x hit lies in [0, 1]: its clamp is reached only as a tie, on both ends; roughness likewise
            assert int((dh['hw_hi'][1] == 0).sum()) > 0 and int((dh['hw_lo'][1] == 0).sum()) > 0
            assert int((dh['r_lo'][1] == 0).sum()) > 0 and int((dh['r_hi'][1] == 0).sum()) > 0
            assert min(_sides(dh, 'hw_hi')) == 0 and min(_sides(dh, 'hw_lo')) == 0
            for k in ('Ld', 'Ls', 'Li'):
                assert bool((s[k][:, :3] == s['exp_max']).any())
            m32 = S.materials(s['m_raw'], s['r_raw'], s['a_raw'])
            assert {0.0, 1.0} <= set(m32[:, 0].tolist()) and {0.0, 1.0} <= set(m32[:, 1].tolist())     # saturated sigmoids, from the raw heads
            assert bool((s['Lh'] == 0).any()) and bool((s['Lh'][:, 3] > 0).any())
            for col, t in ((3, s['geo']), (1, s['mat']), (0, s['mat'])):
                assert bool((t[:, col] == 0).any()) and bool((t[:, col] == 1).any())
            assert len(set(s['ray'].tolist())) >= 2
    print('closest approaches', approach)


def test_nerf_and_composite_inputs_cover_every_branch():
    for n in (1, 63, 64, 65, 127, 128, 129, 200):
        q = S.nerf_inputs(n)
        dec = S.nerf_head(q['sig4'][:, 0].double(), q['rgb4'][:, :3].double(), q['dist'].double())[2]
        d32 = S.nerf_head(q['sig4'][:, 0], q['rgb4'][:, :3], q['dist'])[2]
        assert all(torch.equal(dec[k][0], d32[k][0]) for k in dec)          # direct inputs: decided alike
        if n >= 63:
            assert min(_sides(dec, 'softplus')) > 0 and min(_sides(dec, 'rgb5')) > 0 and min(_sides(dec, 'dist0')) > 0
            assert bool((q['sig4'][:, 0] == 20).any()) and bool((q['rgb4'][:, :3] == 5).any())
            e = torch.exp(torch.clamp(q['rgb4'][:, :3].double(), max=5.0))
            assert bool((e <= 0.0031308).any()) and float((e - 0.0031308).abs().min()) > 1e-5      # the knee inside the head, with margin
    for T in COMPOSITE_WAVE_T + COMPOSITE_THREAD_T:
        for R in (S.WAVE_R if T <= 192 else S.THREAD_R):
            q = S.composite_inputs(R, T)
            dec = S.composite(q['alpha'].double(), q['color'].double())[2]
            assert _close(S.composite(q['alpha'].double(), q['color'].double())[0], O.transmittance_weights(q['alpha'].double()), 1e-13)
            assert _sides(dec, 'opaque')[0] > 0 and (T < 3 or _sides(dec, 'clear')[0] > 0)
            assert float(q['alpha'][0, 0]) == 1.0 and (T < 2 or float(q['alpha'][0, 1]) == float(torch.tensor(0.9999999)))


def test_fp32_autograd_of_opaque_rows_stays_near_fp64():
    """the premise of the 3x-floor rule on the opaque-sample rows: float32 autograd of the reference stays within ~6e-7 of float64 on d_alpha
    of order 1 (alpha = 1.0 followed by 0.9999999)"""
    for T in (1, 64, 65, 193):
        q = S.composite_inputs(3, T)
        g64 = S.composite_bwd(q['alpha'], q['color'], q['d_rgb'])[0]
        g32 = S.composite_bwd(q['alpha'], q['color'], q['d_rgb'], dtype=torch.float32)[0]
        err = (g32.double() - g64).abs() / g64.abs().clamp(min=1.0)
        assert float(err.max()) < 5e-6, (T, float(err.max()))
