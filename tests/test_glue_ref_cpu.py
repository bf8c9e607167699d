"""CPU tier: pins tests/glue_ref.py -- the restatement tests/test_step_glue_kernels_gpu.py compares the step-glue kernels with -- without
a GPU: (1) the select contract written in numpy equals the torch.nonzero / argsort(stable) / sort expression of tests/test_step_glue.py on
every committed case; (2) the loss restatement equals NeROShapeRenderer.compute_rgb_loss + F.l1_loss + the means in float64; (3) every case
is the case its name claims (total against cap, scan blocks and loss blocks against 256, the special rows, the +inf keys); (4) the float32
restatement meets, on every committed input set, the bounds the kernels are held to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_ref as G

F32, F64 = G.F32, G.F64


# ---- nero_occ_select ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(G.SELECT_CASES))
def test_select_contract_equals_the_tensor_expression(name):
    n, cap = G.SELECT_CASES[name][:2]
    flag, keys = G.select_inputs(name)
    cand, (kept, total) = G.occ_select(flag, keys, cap)
    tf, tk = torch.from_numpy(flag), torch.from_numpy(keys)
    ref = torch.nonzero(tf)[:, 0]
    Pn = ref.numel()
    if Pn > cap:
        ref = ref[torch.sort(torch.argsort(tk[:Pn], stable=True)[:cap])[0]]
    assert (kept, total) == (ref.numel(), Pn)
    assert np.array_equal(cand[:kept], ref.numpy()) and bool((cand[kept:] == -1).all()) and cand.shape == (cap,) and cand.dtype == np.int32
    assert bool((np.diff(cand[:kept]) > 0).all()) and (kept == 0 or (0 <= cand[0] and cand[kept - 1] < n))


@pytest.mark.parametrize('name', sorted(G.SELECT_CASES))
def test_select_case_is_what_its_name_says(name):
    n, cap, layout, kset, total_rel, blocks_rel = G.SELECT_CASES[name]
    flag, keys = G.select_inputs(name)
    assert flag.shape == keys.shape == (n,) and flag.dtype == np.uint8 and keys.dtype == np.float32 and 1 <= cap <= G.PICK_MAX
    total = int(np.count_nonzero(flag))
    assert {'zero': total == 0, 'below': 0 < total < cap, 'equal': total == cap, 'plus1': total == cap + 1, 'above': total > cap + 1}[total_rel], total
    nb = -(-n // G.SB)
    assert {'<': nb < G.LB, '==': nb == G.LB, '>': nb > G.LB}[blocks_rel], nb
    assert G.scan_rounds(n) == (2 if blocks_rel == '>' else 1)
    every = np.nonzero(flag)[0]
    if layout == 'first':
        assert every.tolist() == [0]
    if layout == 'last':
        assert every.tolist() == [n - 1]
    if layout == 'last_block':
        assert every.min() >= (nb - 1) * G.SB and n - (nb - 1) * G.SB > 1
    if layout.startswith('from:'):
        assert every.min() >= int(layout.split(':')[1]) >= G.LB * G.SB        # only blocks the SECOND scan round owns
        assert len({int(i) // G.SB for i in every}) > 1
    if layout.startswith('bytes'):
        assert {1, 2, 255} <= set(np.unique(flag).tolist())
    if kset == 'ties16':
        assert len(np.unique(keys)) <= 16
    if kset == 'equal':
        assert len(np.unique(keys)) == 1
    if kset == 'signed_zeros':
        k = keys[:total]
        assert bool((np.signbit(k) & (k == 0)).any()) and bool((~np.signbit(k) & (k == 0)).any()) and int((k == 0).sum()) > cap


def test_select_table_covers_the_sizes_caps_and_layouts():
    ns, caps = {c[0] for c in G.SELECT_CASES.values()}, {c[1] for c in G.SELECT_CASES.values()}
    assert {1, 1023, 1024, 1025, 4097, 262144, 262145, 263169} <= ns and {1, 2, 3, 100, 4095, 4096} <= caps
    assert -(-263169 // G.SB) == 258 and -(-262145 // G.SB) == 257
    layouts = {c[2].split(':')[0] for c in G.SELECT_CASES.values()}
    assert {'none', 'all', 'first', 'last', 'last_block', 'exact', 'plus1', 'bytes', 'frac'} <= layouts
    assert {'random', 'ties16', 'equal'} <= {c[3] for c in G.SELECT_CASES.values()}
    assert {c[4] for c in G.SELECT_CASES.values()} == {'zero', 'below', 'equal', 'plus1', 'above'}
    inf = {k for k, c in G.SELECT_CASES.items() if c[3].startswith(('inf', 'nan'))}
    assert inf == set(G.INF_SHORT) | set(G.INF_LONG) and not set(G.INF_SHORT) & set(G.INF_LONG)


@pytest.mark.parametrize('name', sorted(G.SELECT_CASES))
def test_inf_key_cases_reach_into_the_inf_keys(name):
    """a +inf case named `fewer` really keeps candidates whose key is not finite, and only those cases tell the contract from a sort that
    keys the non-candidates with a float +inf; every other case is one on which the two rules agree"""
    cap = G.SELECT_CASES[name][1]
    flag, keys = G.select_inputs(name)
    cand, (kept, total) = G.occ_select(flag, keys, cap)
    finite = int(np.isfinite(keys[:total]).sum())
    other = G.occ_select_inf_for_the_rest(flag, keys, cap)
    if name in G.INF_SHORT:
        assert finite < kept, (finite, kept)
        assert other[1] == (kept, total) and not np.array_equal(other[0], cand)
    else:
        assert finite >= kept and (name not in G.INF_LONG or (cap < finite < total))
        assert other[1] == (kept, total) and np.array_equal(other[0], cand)
    if name == 'inf_issue_example_cap4':
        assert cand.tolist() == [1, 3, 4, 7] and other[0].tolist() == [0, 1, 2, 3]
    if name == 'inf_total_below_cap100':
        assert total <= cap
    if name == 'inf_finite_keys_on_the_last_candidates_cap100':
        assert bool(np.isinf(keys[:total - 20]).all()) and bool(np.isfinite(keys[total - 20:total]).all())
    if name == 'inf_then_nan_keys_cap100':
        assert int(np.isinf(keys[:total]).sum()) == 20 and int(np.isnan(keys[:total]).sum()) == total - 50 and kept > 50


# ---- nero_near_far_sphere -------------------------------------------------------------------------------------------------------------
def test_near_far_rays_are_the_kinds_they_are_named():
    from nero_amd.renderer import NeROShapeRenderer
    assert G.NEAR_FAR_R == (1, 255, 256, 257, 1000)
    seen = set()
    for R, s in G.near_far_family():
        q = G.near_far_inputs(R, s)
        o, d, kind = q['o'].double(), q['d'].double(), q['kind']
        assert q['o'].dtype == F32 and q['o'].shape == q['d'].shape == (R, 3)
        seen |= set(kind.tolist())
        k = lambda nm: kind == G.RAY_KINDS.index(nm)
        dn, on = d.norm(dim=-1), o.norm(dim=-1)
        assert bool(((dn[k('unit')] - 1).abs() < 1e-6).all()) and bool(((dn[k('dir_x1e-3')] / 1e-3 - 1).abs() < 1e-6).all())
        assert bool(((dn[k('dir_x1e3')] / 1e3 - 1).abs() < 1e-6).all())
        for nm, v in (('unit', 3.0), ('origin_1e-3', 1e-3), ('origin_on_sphere', 1.0), ('origin_1e3', 1e3), ('inside_half', 0.5)):
            assert bool(((on[k(nm)] / v - 1).abs() < 1e-6).all()), nm
        c = k('through_centre')
        assert bool((torch.cross(o[c], d[c], dim=-1).norm(dim=-1) < 1e-6).all())
        p = k('perpendicular')
        assert bool((((o * d).sum(-1).abs() / (on * dn))[p] < 2e-4).all())                       # o.d cancels: 1e-4 of |o| |d| is left
        n64, f64, unit = G.near_far(q['o'], q['d'])
        n32, f32, _ = G.near_far(q['o'], q['d'], F32)
        inside = (kind == G.INSIDE[0]) | (kind == G.INSIDE[1])
        assert bool((n64[inside] == G.NEAR_MIN).all()) and bool((n32[inside] == np.float32(1e-3)).all())
        assert bool((unit >= 1).all())
        # the restatement is near_far_from_sphere (whose clamp constant is the double 1e-3)
        rn, rf = NeROShapeRenderer.near_far_from_sphere(o, d)
        assert float((rn[:, 0] - n64).abs().max()) <= 1e-10 and torch.equal(rf[:, 0], f64)
        fl = G.near_far_floors()
        assert G.row_err(n32, n64, unit) <= G.bound_of(fl['near']) and G.row_err(f32, f64, unit) <= G.bound_of(fl['far'])
    assert seen == set(range(len(G.RAY_KINDS)))
    assert 0 < G.near_far_floors()['near'] < 1e-5 and 0 < G.near_far_floors()['far'] < 1e-5


# ---- nero_occ_gather / nero_occ_l1 ----------------------------------------------------------------------------------------------------
def test_gather_and_l1_cases():
    assert {c for c, _ in G.GATHER_CASES} == {1, 255, 256, 257}
    for cap, variant in G.GATHER_CASES:
        q = G.gather_inputs(cap, variant)
        both = torch.cat([q['x4'].reshape(-1), q['geo'].reshape(-1)])
        assert both.unique().numel() == both.numel()                       # a wrong row, column or stride shows
        cand = q['cand']
        used = cand >= 0
        assert bool((cand[used][1:] > cand[used][:-1]).all()) and int(cand.max()) < q['x4'].shape[0]
        if variant == 'holes':
            assert int(cand[-1]) == -1
            if cap > 5:
                last = int(torch.nonzero(used)[-1])
                assert bool((~used[:last]).any())                             # -1 in the middle too
        pts, dirs = G.occ_gather(q['x4'], q['geo'], cand)
        assert bool((pts[~used] == 0).all()) and bool((dirs[~used] == torch.tensor([0.0, 0.0, 1.0])).all())
    assert {c[0] for c in G.L1_CASES} == {1, 1023, 1024, 1025, 4096} and {c[2] for c in G.L1_CASES} == {1, 4097, 70001}
    for cap in {c[0] for c in G.L1_CASES}:
        kepts = {c[1] for c in G.L1_CASES if c[0] == cap}
        assert cap in kepts and kepts <= {cap, cap // 3, 1, 0}
    assert {0, 1} <= {c[1] for c in G.L1_CASES} and any(c[1] == c[0] // 3 and c[1] > 1 for c in G.L1_CASES)
    for case in G.L1_CASES:
        cap, kept, n_in = case
        q = G.l1_inputs(*case)
        assert int((q['cand'] >= 0).sum()) == kept == int(q['counts'][0]) and (kept > 0 or q['counts'].tolist() == [0, 0])
        l64, g64 = G.occ_l1_fwd_bwd(q)
        l32, g32 = G.occ_l1_fwd_bwd(q, F32)
        assert int((g64 != 0).sum()) == max(kept - (kept >= 2), 0)         # the tie has gradient exactly 0
        if kept == 0:
            assert float(l64) == 0.0 and float(l32) == 0.0
        assert G.rel(l32, l64) <= G.loss_bound(max(kept, 1)) and G.row_err(g32, g64) <= G.bound_of(G.l1_floor())


# ---- nero_shape_loss --------------------------------------------------------------------------------------------------------------------
def test_loss_shapes_are_what_they_are_for():
    assert G.LOSS_SHAPES[:7] == [(1, 0), (1, 1), (255, 257), (257, 255), (256, 256), (700, 65793), (66000, 300)]
    blocks = {s: -(-max(s) // G.LB) for s in G.LOSS_SHAPES}
    assert blocks[(700, 65793)] > G.LB and blocks[(66000, 300)] > G.LB and blocks[(300, 65537)] == G.LB + 1
    assert all(b <= 2 for s, b in blocks.items() if max(s) <= 257)
    assert G.loss_rounds(65793) == 2 and G.loss_rounds(66000) == 2 and G.loss_rounds(65537) == 2 and G.loss_rounds(65536) == 1
    assert G.scan_rounds(262144) == 1 and G.scan_rounds(262145) == 2
    assert G.loss_bound(300) == 23 * G.EPS32 and G.loss_bound(66000) == 24 * G.EPS32
    assert G.occ_modes(0) == ['none'] and G.occ_modes(1) == ['none', 'kept0', 'kept1'] and G.occ_modes(300) == list(G.OCC_MODES)
    for R, n_in, mode in G.loss_family():
        q = G.loss_inputs(R, n_in, mode)
        df = q['rgb'] - q['gt']                                          # float32, as the kernel forms it
        if R >= 3:
            assert bool((df[0] == 0).all()) and df[1].tolist() == [0.25, -0.25, 0.25] and df[2].tolist() == [-0.25, 0.25, -0.25]
            assert bool((df.double()[1:3] == (q['rgb'].double() - q['gt'].double())[1:3]).all())       # exactly representable
        if mode == 'none':
            assert q['cand'] is None
        else:
            kept = int(q['counts'][0])
            assert kept == {'kept0': 0, 'kept1': 1, 'full': G.LOSS_CAP}[mode] == int((q['cand'] >= 0).sum()) and q['cand'].numel() == G.LOSS_CAP
            if mode == 'full':
                assert int((q['occ'][q['cand'].long()] == q['gt_occ']).sum()) == 1


@pytest.mark.parametrize('kind', range(4), ids=G.KINDS)
def test_loss_restatement_is_the_renderers_loss_and_float32_meets_the_bounds(kind):
    from nero_amd.renderer import NeROShapeRenderer

    class Net:
        cfg = {'rgb_loss': G.KINDS[kind]}
    floors = G.loss_floors(kind)
    assert all(0 <= v < 1e-5 for v in floors.values())
    for R, n_in, mode in G.loss_family():
        q = G.loss_inputs(R, n_in, mode)
        bounds = G.loss_bounds(R, n_in, mode)
        for wi, w in enumerate(G.WEIGHTS):
            losses, d_rgb, d_gerr, d_occ = G.loss_refs(R, n_in, mode, kind, wi)
            a, b, c = G.leaf(q['rgb'], F64), G.leaf(q['gerr'], F64), G.leaf(q['occ'], F64)
            w0, w1 = (1.0, 1.0) if w is None else w
            want = [NeROShapeRenderer.compute_rgb_loss(Net, a, q['gt'].double()).mean(), torch.zeros((), dtype=F64), torch.zeros((), dtype=F64)]
            if n_in:
                want[1] = (b * G.EIK_W).mean() * w0
            kept = 0 if q['cand'] is None else int(q['counts'][0])
            if kept:
                want[2] = F.l1_loss(c[q['cand'][:kept].long()], q['gt_occ'][:kept].double()) * w1
            total = want[0] + want[1] + want[2]
            gs = torch.autograd.grad(total, [a, b, c], allow_unused=True)
            ref = torch.stack([total] + want).detach()
            assert float((losses - ref).abs().max()) <= 1e-15 * max(1.0, float(ref.abs().max())), (R, n_in, mode, wi)
            for got, g_, leaf_ in zip((d_rgb, d_gerr, d_occ), gs, (a, b, c)):
                g_ = torch.zeros_like(leaf_) if g_ is None else g_
                assert float((got - g_).abs().max() if got.numel() else 0.0) <= 1e-18, (R, n_in, mode, wi)
            assert int((d_occ != 0).sum()) == max(kept - (kept >= 2), 0)
            # the float32 restatement against the bounds of the kernels
            l32, r32, g32, o32 = G.loss_refs(R, n_in, mode, kind, wi, F32)
            for i in range(4):
                if bounds[i] == 0.0:
                    assert float(l32[i]) == 0.0 == float(losses[i])
                else:
                    assert G.rel(l32[i], losses[i]) <= bounds[i], (R, n_in, mode, wi, i, G.rel(l32[i], losses[i]), bounds[i])
            for nm, x32, x64 in (('d_rgb', r32, d_rgb), ('d_gerr', g32, d_gerr), ('d_occ', o32, d_occ)):
                assert G.row_err(x32, x64) <= G.bound_of(floors[nm]), (nm, R, n_in, mode, wi)


# ---- nero_var_grad ------------------------------------------------------------------------------------------------------------------------
def test_var_grad_cases_stay_clear_of_the_gate():
    v, s = G.var_grad_inputs()
    assert len(G.VARIANCES) == 64 and np.float32(0.3) in G.VARIANCES and min(G.VARIANCES) == np.float32(-1.3) and max(G.VARIANCES) == np.float32(1.3)
    assert bool(((v.double().abs() - G.GATE).abs() > 1e-3).all()) and bool((s > 0).any()) and bool((s < 0).any())
    g64, g32 = G.var_grad(s, v), G.var_grad(s, v, F32)
    live = torch.tensor([abs(float(x)) < G.GATE for x in v])
    assert torch.equal(g64 != 0, live) and torch.equal(g32 != 0, live) and int((~live).sum()) == 2 * len(G.DSUMS)
    for x, is_live in G.GATE_VARIANCES:
        assert (abs(float(x)) < G.GATE) == is_live
    want = s.double() * 10.0 * torch.exp(10.0 * v.double())
    assert float(((g64 - want).abs() / want.abs())[live].max()) <= 1e-15
    assert G.row_err(g32, g64) <= G.bound_of(G.var_grad_floor())
