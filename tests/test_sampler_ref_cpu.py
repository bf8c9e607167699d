"""CPU tier: pins tests/sampler_ref.py, the plain restatement the GPU tier (tests/test_sampler_kernels_gpu.py) compares the sampler
and ray-preparation kernels with.  No GPU, no project kernel."""
import functools

import pytest
import torch

from oracle import nero_oracle as O
from tests import sampler_ref as SR
from tests.helpers import T, build_case_model, load_golden


@functools.lru_cache(maxsize=None)
def _golden_trace(name='bell_s25000'):
    z, meta = load_golden(name)
    net = build_case_model(meta)
    P = O.effective_params({k: v.detach() for k, v in net.state_dict().items()})
    cfg = {**O.DEFAULT_CFG, **meta['cfg']}
    trace = []
    zv = O.sample_ray(P, cfg, T(z, 'o'), T(z, 'd'), T(z, 'near'), T(z, 'far'), T(z, 'rand1'), T(z, 'rand_bg'), trace)
    return z, cfg, P, trace, zv


def test_reference_agrees_with_oracle_sample_ray_on_golden_case():
    z, cfg, P, trace, zv = _golden_trace()
    o, d = T(z, 'o'), T(z, 'd')
    ns, nb = cfg['n_samples'], cfg['n_bg_samples']
    assert torch.equal(SR.coarse_z(T(z, 'near'), T(z, 'far'), ns, T(z, 'rand1')), trace[0]['z'])
    assert torch.equal(SR.background_z(T(z, 'far'), nb, T(z, 'rand_bg')), zv[:, -nb:])
    for i, t in enumerate(trace):
        # the plain two-pointer merge is the oracle's stable sort, and the golden permutation dumped from the reference
        zm, index = SR.merge_two_pointer(t['z'], t['z_new'])
        assert torch.equal(zm, t['z_out']) and torch.equal(index, t['index'])
        assert torch.equal(index, T(z, f'tr/index{i}').long())
        w = SR.upsample_weights(o, d, t['z'], t['sdf'], t['inv_s'])
        assert torch.equal(w, t['weights'])
        zn, inds = SR.sample_pdf_det(t['z'], w, t['z_new'].shape[1])
        assert torch.equal(inds, T(z, f'tr/inds{i}').long()) and torch.equal(zn, t['z_new'])
        cos, inside = SR.upsample_parts(o, d, t['z'], t['sdf'])
        assert cos.shape == inside.shape == w.shape
    # render preparation on the reference's own z_vals: the inner count is the length of its per-inner-sample output
    rp = SR.render_prep(o, d, T(z, 'z_vals'))
    assert rp['counts'][0] == z['gradient_error'].shape[0] and sum(rp['counts']) == T(z, 'z_vals').numel()
    # ... and the float32 statement of pts4 is the oracle's point expression, bit for bit
    zv_ = T(z, 'z_vals')
    dists = torch.cat([zv_[:, 1:] - zv_[:, :-1], (zv_[:, 1:] - zv_[:, :-1])[:, -1:]], -1)
    pts = (o[:, None, :] + d[:, None, :] * (zv_ + dists * 0.5)[..., None]).reshape(-1, 3)
    p4 = SR.render_prep_f32(o, d, zv_)
    assert torch.equal(p4[:, :3], pts) and torch.equal(p4[:, 3], dists.reshape(-1))
    assert torch.equal(SR.inner_mask_f32(p4), rp['inner'].reshape(-1))


def test_section_weights_and_occ_march_agree_with_the_oracle():
    z, cfg, P, _, _ = _golden_trace()
    g = torch.Generator().manual_seed(3)
    p = torch.nn.functional.normalize(torch.randn(37, 3, generator=g), dim=-1) * torch.rand(37, 1, generator=g) * 0.8
    dd = torch.nn.functional.normalize(torch.randn(37, 3, generator=g), dim=-1)
    zz = SR.occ_z(p, dd, 64)
    assert torch.equal(zz, O.sphere_exit_dist(p, dd) * torch.linspace(0, 1, 64)[None, :])
    assert float(zz[:, 0].abs().max()) == 0.0 and bool((zz[:, 1:] > zz[:, :-1]).all())
    # the march ends on the unit sphere
    assert float((torch.linalg.norm(p.double() + dd.double() * SR.occ_z(p.double(), dd.double(), 64)[:, -1:], dim=-1) - 1).abs().max()) < 1e-6
    pts = zz.unsqueeze(-1) * dd.unsqueeze(-2) + p.unsqueeze(-2)
    with torch.no_grad():
        sdf = O.sdf_network(P, pts.reshape(-1, 3))[:, 0].reshape(zz.shape)
        w_o, _ = O.section_weights(P, zz, p, dd, 20.0)
    w, cos = SR.section_weights(zz, sdf, 20.0)
    assert torch.equal(w, w_o)
    assert bool((w[cos >= 0] == 0).all()) and bool((cos >= 0).any()) and bool((cos < 0).any())


@pytest.mark.parametrize('n,m', [(2, 1), (63, 1), (64, 16), (65, 32), (128, 32), (129, 31), (150, 10)])
def test_stable_sort_merge_is_the_two_pointer_merge_with_old_first_ties(n, m):
    z, zn = SR.tie_merge_inputs(9, n, m)
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((zn[:, 1:] >= zn[:, :-1]).all())
    # the inputs do hold ties: new values equal to old ones, and (m >= 3) equal neighbours inside z_new
    assert bool((zn[:, :, None] == z[:, None, :]).any(-1).any(-1).all())
    assert m < 3 or bool((zn[:, 1:] == zn[:, :-1]).any(-1).all())
    sdf, sdf_new = torch.arange(9 * n).reshape(9, n).float(), -1.0 - torch.arange(9 * m).reshape(9, m).float()
    zs, s, index = SR.merge_sorted(z, sdf, zn, sdf_new)
    zm, im = SR.merge_two_pointer(z, zn)
    assert torch.equal(zs, zm) and torch.equal(index, im)
    assert torch.equal(s, torch.gather(torch.cat([sdf, sdf_new], -1), -1, im))
    # old first on ties: among equal values every old element precedes every new one
    old = index < n
    same = zs[:, 1:] == zs[:, :-1]
    assert not bool((same & ~old[:, :-1] & old[:, 1:]).any())


@pytest.mark.parametrize('n,m', [(160, 32), (128, 32), (65, 32)])
def test_three_spikes_reach_the_small_denominator_branch(n, m):
    z, w = SR.three_spikes(2000, n, seed=1)
    count = SR.small_denominators(z, w, m)
    zn, inds = SR.sample_pdf_det(z, w, m)
    assert count > 0, 'the recipe no longer reaches denom < 1e-5: the GPU tier would not exercise that branch'
    assert bool(torch.isfinite(zn).all()) and int(inds.min()) >= 1 and int(inds.max()) <= n
    # the rows the GPU tier runs: the first of them take the branch
    zr, wr = SR.spike_rows(5, n, m)
    assert bool(SR.small_denominator_rows(zr, wr, m)[0]) and SR.small_denominators(zr, wr, m) > 0
    # all-zero weights: a uniform pdf, still finite and in range
    zu, iu = SR.sample_pdf_det(z[:3], torch.zeros(3, n - 1), m)
    assert bool(torch.isfinite(zu).all()) and bool((zu >= z[:3, :1]).all()) and bool((zu <= z[:3, -1:]).all())


@pytest.mark.parametrize('T_', [1, 2, 65, 193])
def test_render_prep_compact_and_scan_are_consistent(T_):
    g = torch.Generator().manual_seed(5)
    R = 23
    o, d, near, far = SR.rays_through_sphere(R, g)
    z = torch.sort(near + (far - near) * 1.6 * torch.rand(R, T_, generator=g), -1)[0]
    rp = SR.render_prep(o, d, z)
    inner_idx, outer_idx = SR.compact(rp['inner'])
    assert (inner_idx.numel(), outer_idx.numel()) == rp['counts']
    assert torch.equal(torch.sort(torch.cat([inner_idx, outer_idx]))[0], torch.arange(R * T_))
    if T_ > 1:
        assert torch.equal(rp['dist'][:, -1], rp['dist'][:, -2]) and torch.equal(rp['dist'][:, :-1], z[:, 1:] - z[:, :-1])
        assert 0 < rp['counts'][0] < R * T_
    else:
        assert float(rp['dist'].abs().max()) == 0.0
    for r in range(R):
        # the exclusive offsets index the compacted lists: ray r's inner samples start at ray_off[r], its outer ones at r*T - ray_off[r]
        a, c = int(rp['ray_off'][r]), int(rp['ray_counts'][r])
        assert torch.equal(inner_idx[a:a + c], r * T_ + torch.nonzero(rp['inner'][r])[:, 0])
        b = r * T_ - a
        assert torch.equal(outer_idx[b:b + T_ - c], r * T_ + torch.nonzero(~rp['inner'][r])[:, 0])
    assert int(rp['ray_off'][0]) == 0 and int(rp['ray_off'][-1] + rp['ray_counts'][-1]) == rp['counts'][0]


def test_encoding_rows_layout():
    g = torch.Generator().manual_seed(7)
    p = torch.randn(5, 3, generator=g, dtype=torch.float64)
    pe = SR.pe6_rows(p)
    assert pe.shape == (64, 40) and torch.equal(pe[:5, :39], O.pos_enc(p, 6)) and float(pe[5:].abs().max()) == 0 and float(pe[:, 39].abs().max()) == 0
    assert torch.equal(pe[:5, 3 + 6 * 2:6 + 6 * 2], torch.sin(4 * p)) and torch.equal(pe[:5, 6 + 6 * 5:9 + 6 * 5], torch.cos(32 * p))
    p4 = SR.outer_point(p)
    assert float((torch.linalg.norm(p4[:, :3], dim=-1) - 1).abs().max()) < 1e-15
    assert float((p4[:, 3] * torch.linalg.norm(p, dim=-1) - 1).abs().max()) < 1e-15
    pe88 = SR.pe10_rows88(p4, 64)
    assert pe88.shape == (64, 88) and float(pe88[:, 84:].abs().max()) == 0
    assert torch.equal(pe88[:5, 4 + 8 * 4:8 + 8 * 4], torch.sin(16 * p4))              # frequency 4 closes the first 44 columns
    assert torch.equal(pe88[:5, 44:48], torch.sin(32 * p4)) and torch.equal(pe88[:5, 80:84], torch.cos(512 * p4))
    w = SR.view_dir(p)
    pv = SR.pe4_rows32(w, 64)
    assert pv.shape == (64, 32) and float(pv[:, 27:].abs().max()) == 0 and torch.equal(pv[:5, :3], w)
    assert torch.equal(pv[:5, 24:27], torch.cos(8 * w)) and float((torch.linalg.norm(w, dim=-1) - 1).abs().max()) < 1e-15
    assert SR.row_pad(0) == 0 and SR.row_pad(1) == 64 and SR.row_pad(64) == 64 and SR.row_pad(65) == 128


def test_occ_candidates_predicate():
    x = torch.tensor([[0.5, 0, 0], [0.9995, 0, 0], [0.5, 0, 0], [0.5, 0, 0]], dtype=torch.float64)
    sdf = torch.tensor([0.001, 0.001, 0.02, 0.001], dtype=torch.float64)
    grad = torch.tensor([[1.0, 0, 0]] * 4, dtype=torch.float64)
    d = torch.tensor([[-3.0, 0, 0], [-3.0, 0, 0], [-3.0, 0, 0], [2.0, 0, 0]], dtype=torch.float64)
    flag, margin = SR.occ_candidates(x, sdf, grad, d, 0.01)
    assert flag.tolist() == [True, False, False, False] and bool((margin > 1e-4).all())


def test_sample_positions_are_stated_element_by_element():
    """u = linspace(0.5/m, 1 - 0.5/m, m) of the inverse-CDF sampling, float32: the oracle's explicit statement is the scalar float32
    recurrence (every operation rounded on its own), equals torch.linspace where the step is exact (m a power of two: the YAML and golden
    shapes) and stays within rounding of it elsewhere"""
    import numpy as np
    f = np.float32
    for m in range(1, 33):
        u0 = f(f(0.5) / f(m))
        u1 = f(f(1.0) - u0)
        step = f(f(u1 - u0) / f(m - 1)) if m > 1 else f(0)
        want = [f(u0 + f(step * f(i))) if i < m // 2 else f(u1 - f(step * f(m - 1 - i))) for i in range(m)] if m > 1 else [u0]
        t0 = torch.tensor(0.5) / m
        got = O.linspace_sym(t0, 1.0 - t0, m, torch.float32)
        assert np.array_equal(got.numpy(), np.array(want, f)), m
        lin = torch.linspace(0.5 / m, 1.0 - 0.5 / m, m, dtype=torch.float32)
        # (both are at most 3 roundings of values below 1 away from the exact value: 6 x 2^-24 apart at the most, whatever the host's ATen does)
        assert float((got - lin).abs().max()) <= 6 * 2.0 ** -24, m
        if m & (m - 1) == 0:
            assert torch.equal(got, lin), m
    # float64 (the oracle's other dtype): the same statement, to the last bits of torch.linspace
    assert float((O.linspace_sym(0.0, 1.0, 64, torch.float64) - torch.linspace(0, 1, 64, dtype=torch.float64)).abs().max()) < 1e-15
