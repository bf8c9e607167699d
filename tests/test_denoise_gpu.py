"""GPU tier of the denoiser (include/nero_hip_denoise.h, nero_amd/csrc/denoise.hip, nero_amd/denoise.py, Relighter.render(denoise=...)):
both entry points and the whole denoise() against the float64 restatement (tests/denoise_ref.py) within 4 float32 floors, the cases that
are exact by arithmetic, bit-stability, and the relighter end to end against a converged render."""
import numpy as np
import pytest
import torch

from tests import denoise_ref as DR

pytestmark = pytest.mark.gpu
K_FLOOR = 4.0                                                       # the bound: 4 x the restatement's own float32-to-float64 distance
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (17, 33), (40, 48), (64, 64)]              # 5 x 3 and smaller lie within the reach of step 16 (32 pixels)
COMBOS = [(0, 6), (4, 6), (0, 0), (4, 0), (0, 10), (4, 10)]                          # (G, k)
SIG = dict(sigma_l=4.0, sigma_p=0.05, sigma_g=0.1)


@pytest.fixture(scope='module')
def DN():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import denoise
    return denoise


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_SCENES = {}


def _scene(h, w):
    """the analytic scene at h x w with a tenth of its pixels uncovered (none of 1 x 1), computed once"""
    if (h, w) not in _SCENES:
        _SCENES[h, w] = DR.sphere_over_plane(h, w, noise=0.5, seed=1, frame=0, holes=0.1 if h * w > 1 else 0.0)
    return _SCENES[h, w]


def _ref_denoise(rgb, sc, valid, h, w, dt, **kw):
    """the restatement's denoise() as one [n,4] array (rgb, variance)"""
    out, var = DR.denoise(rgb, sc['pos'], sc['normal'], valid, h, w, dtype=dt, **kw)
    return np.concatenate([out, var[:, None]], 1)


def _held(name, got, ref32, ref64):
    """rgb and variance each against their own scale -> the worst (error, floor) pair by ratio, asserted"""
    worst = 0.0
    for what, cols in (('rgb', slice(0, 3)), ('var', slice(3, 4))):
        if ref64.shape[1] <= cols.start:
            continue
        err, floor = DR.parity(got[:, cols], ref32[:, cols], ref64[:, cols])
        ratio = err / floor if floor > 0 else (0.0 if err == 0 else float('inf'))
        print(f'{name} {what}: kernel {err:.3e} floor {floor:.3e} ({ratio:.2f} floors)')
        assert err <= K_FLOOR * floor, (name, what, err, floor)
        worst = max(worst, ratio)
    return worst


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G,k', COMBOS)
@pytest.mark.parametrize('h,w', SHAPES)
def test_parity_with_the_float64_restatement(DN, h, w, G, k):
    """the variance pass, the a-trous pass at steps 1, 2 and 16 and the whole denoise() on the noisy analytic scene: the kernels' distance
    from the float64 restatement is at most 4 x the float32 restatement's, relative to max(|value|, mean |value|), for rgb and for the
    variance.  Every pass is given the same float32 input in all three."""
    sc = _scene(h, w)
    extra = sc['extra'] if G == 4 else None
    guide, sig = DR.pack_guides(sc['pos'], sc['normal'], sc['valid'], extra), DR.pack_signal(sc['noisy'])
    g_dev = _cu(guide)
    name = f'{h}x{w} G={G} k={k}'
    ref = {dt: DR.estimate_variance(guide, sig, h, w, k, SIG['sigma_p'], SIG['sigma_g'], dtype=dt) for dt in (np.float32, np.float64)}
    got = DN.estimate_variance(g_dev, _cu(sig), h, w, k, SIG['sigma_p'], SIG['sigma_g'])
    worst = _held(name + ' variance', got.cpu().numpy(), ref[np.float32], ref[np.float64])
    with_var = ref[np.float32]                                        # float32: the same input for all three
    for step in (1, 2, 16):
        ref = {dt: DR.atrous_pass(guide, with_var, h, w, step, k, dtype=dt, **SIG) for dt in (np.float32, np.float64)}
        got = DN.atrous_pass(g_dev, _cu(with_var), h, w, step, k, **SIG)
        worst = max(worst, _held(f'{name} step {step}', got.cpu().numpy(), ref[np.float32], ref[np.float64]))
    ref = {dt: _ref_denoise(sc['noisy'], sc, sc['valid'], h, w, dt, extra=extra, normal_pow2=k, **SIG) for dt in (np.float32, np.float64)}
    rgb, var = DN.denoise(_cu(sc['noisy']), _cu(sc['pos']), _cu(sc['normal']), _cu(sc['valid']), h, w, None if extra is None else _cu(extra), 5,
                          normal_pow2=k, **SIG)
    got = torch.cat([rgb, var[:, None]], 1).cpu().numpy()
    worst = max(worst, _held(name + ' denoise', got, ref[np.float32], ref[np.float64]))
    print(f'{name}: worst {worst:.2f} floors')


# ---- 2. exact cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G', [0, 4])
def test_an_image_with_no_valid_pixel_comes_back_bit_for_bit(DN, G):
    h, w = 17, 33
    g = torch.Generator().manual_seed(3)
    guide = torch.randn(h * w, 8 + G, generator=g).cuda()
    guide[:, 3] = 0.0
    sig = torch.randn(h * w, 4, generator=g).cuda()
    sig[5, 1], sig[9, 3] = float('nan'), float('inf')
    for out in (DN.estimate_variance(guide, sig, h, w), DN.atrous_pass(guide, sig, h, w, 1), DN.atrous_pass(guide, sig, h, w, 4)):
        assert torch.equal(_bits(out), _bits(sig))


def test_a_lone_valid_pixel_is_unchanged_within_the_bound(DN):
    """its only tap is itself: rgb' = (wt rgb) / wt, one rounding each way; the variance of one sample is exactly 0"""
    h, w = 9, 11
    sc = DR.sphere_over_plane(h, w, frame=0)
    valid = np.zeros(h * w, bool)
    valid[4 * w + 5] = True
    rgb, var = DN.denoise(_cu(sc['noisy']), _cu(sc['pos']), _cu(sc['normal']), _cu(valid), h, w, sigma_p=0.05)
    got = np.concatenate([rgb.cpu().numpy(), var.cpu().numpy()[:, None]], 1)
    ref = {dt: _ref_denoise(sc['noisy'], sc, valid, h, w, dt) for dt in (np.float32, np.float64)}
    _held('lone pixel', got, ref[np.float32], ref[np.float64])
    assert np.array_equal(got[~valid, :3], sc['noisy'][~valid]) and not got[:, 3].any()
    # 5 passes x 2 roundings (the product and the quotient) of at most 2^-24 relative each, and room for their second order
    assert np.abs(got[valid, :3] - sc['noisy'][valid]).max() <= 11 * 2.0 ** -24 * np.abs(sc['noisy'][valid]).max()


@pytest.mark.parametrize('hw', [(16, 24), (33, 70)])
def test_perpendicular_halves_do_not_mix(DN, hw):
    """normals exactly (1, 0, 0) on the left and (0, 1, 0) on the right, signals 0 and 1: the cross weights are exactly 0, and on the right
    sum(wt 1) and sum(wt) accumulate the same bits, so every output is exactly 0.0 or exactly 1.0 -- at every iteration"""
    h, w = hw
    sc = DR.sphere_over_plane(h, w, frame=0)
    left = (np.arange(h * w) % w) < w // 2
    nrm = np.where(left[:, None], np.asarray([1.0, 0, 0], np.float32), np.asarray([0, 1.0, 0], np.float32))
    rgb = np.where(left[:, None], 0.0, 1.0).astype(np.float32).repeat(3, 1)
    for it in (1, 5):
        out, var = DN.denoise(_cu(rgb), _cu(sc['pos']), _cu(nrm), torch.ones(h * w).cuda(), h, w, iterations=it, sigma_p=0.05)
        assert torch.equal(_bits(out), _bits(_cu(rgb))) and not var.any()


def test_a_constant_signal(DN):
    """variance exactly 0 (the moments are taken about the centre's luminance); the output within a few ulp of the constant"""
    h, w = 40, 48
    sc = _scene(h, w)
    const = np.tile(np.asarray([[0.3, 0.55, 0.7]], np.float32), (h * w, 1))
    guide = _cu(DR.pack_guides(sc['pos'], sc['normal'], sc['valid'], sc['extra']))
    v = DN.estimate_variance(guide, _cu(DR.pack_signal(const)), h, w)
    assert not v[:, 3].any() and torch.equal(_bits(v[:, :3]), _bits(_cu(const)))
    out, var = DN.denoise(_cu(const), _cu(sc['pos']), _cu(sc['normal']), _cu(sc['valid']), h, w, _cu(sc['extra']), sigma_p=0.05)
    assert not var.any()
    # each pass is a ratio of two 25-term sums of positive terms that differ by the roundings of 25 products and 48 additions: a random walk
    # of some 70 half-ulps, 2 to 3 ulp at the worst pixel, and the next pass averages what it is handed.  5 passes x 3 ulp, rounded up to 16
    # ulp of a value in [0.5, 1) (2^-24 each); the largest channel is 0.7
    drift = float((out - _cu(const)).abs().max())
    print(f'constant signal: drift {drift / 2.0 ** -24:.1f} ulp of 0.7')
    assert drift <= 16 * 2.0 ** -24


# ---- 3. stability ---------------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_twice_and_the_input_untouched(DN):
    h, w = 64, 64
    sc = _scene(h, w)
    guide = _cu(DR.pack_guides(sc['pos'], sc['normal'], sc['valid'], sc['extra']))
    sig = _cu(DR.pack_signal(sc['noisy'], var=np.full(h * w, 0.01)))
    keep, gkeep = sig.clone(), guide.clone()
    runs = [(DN.estimate_variance(guide, sig, h, w), DN.atrous_pass(guide, sig, h, w, 1), DN.atrous_pass(guide, sig, h, w, 8),
             DN.denoise_records(guide, sig, h, w)) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(sig), _bits(keep)) and torch.equal(_bits(guide), _bits(gkeep))
    with pytest.raises(Exception, match='same buffer'):
        DN.atrous_pass(guide, sig, h, w, 1, out=sig)
    assert torch.equal(_bits(sig), _bits(keep))


def test_a_step_beyond_the_image_is_the_centre_tap_alone(DN):
    """every tap but the centre falls outside: the same bits for every such step, up to the largest (2^20), and what the float32
    restatement gives with them; rgb moves by a rounding, the variance becomes var (wt wt) / (wt wt)"""
    h, w = 5, 3
    sc = _scene(h, w)
    guide = DR.pack_guides(sc['pos'], sc['normal'], sc['valid'])
    sig = DR.pack_signal(sc['noisy'], var=np.linspace(0.01, 0.2, h * w))
    outs = [DN.atrous_pass(_cu(guide), _cu(sig), h, w, step) for step in (5, 16, 2 ** 20)]          # 5 x 3: a tap 5 pixels away lies outside
    for o in outs[1:]:
        assert torch.equal(_bits(o), _bits(outs[0]))
    assert not torch.equal(_bits(DN.atrous_pass(_cu(guide), _cu(sig), h, w, 1)), _bits(outs[0]))
    ref = {dt: DR.atrous_pass(guide, sig, h, w, 2 ** 20, dtype=dt) for dt in (np.float32, np.float64)}
    _held('step 2^20', outs[0].cpu().numpy(), ref[np.float32], ref[np.float64])
    assert np.abs(outs[0].cpu().numpy() - sig).max() <= 4 * 2.0 ** -23 * np.abs(sig).max()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def views(DN):
    """an icosphere of radius 0.5 over a ground quad, seen from above at 64 x 64 under a random map with a hot texel: 8+8 samples plain and
    denoised, 512+512 plain and denoised, with and without one bounce -- rendered once"""
    from nero_amd import relight as RL
    from nero_amd.synthetic import icosphere
    from tests import relight_ref as RR
    v, f = icosphere(2, 0.5)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
    q = np.asarray([[-1.2, -1.2, -0.55], [1.2, -1.2, -0.55], [1.2, 1.2, -0.55], [-1.2, 1.2, -0.55]], np.float32)
    f = np.concatenate([f, np.asarray([[0, 1, 2], [0, 2, 3]]) + len(v)])
    nS = len(v)
    v = np.concatenate([v, q])
    on = (np.arange(len(v)) < nS)[:, None]
    mats = {'metallic': np.where(on, 0.1, 0.0).astype(np.float32), 'roughness': np.where(on, 0.5, 0.7).astype(np.float32),
            'albedo': np.where(on, np.asarray([[0.8, 0.4, 0.3]]), np.asarray([[0.5, 0.6, 0.7]])).astype(np.float32)}
    rl = RL.Relighter(v, f, mats, RR.proper_map(16, 32, seed=2, hot=(3, 20, 30.0)), convention='blender')
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(4, 30.0, 40.0, 2.6))[1]
    Km = np.asarray([[80.0, 0, 32], [0, 80.0, 32], [0, 0, 1]], np.float32)
    out = {'rl': rl, 'pose': pose, 'K': Km}
    for b in (0, 1):
        out[b] = {'noisy': rl.render(pose, Km, 64, 64, samples=(8, 8), bounces=b),
                  'noisy_dn': rl.render(pose, Km, 64, 64, samples=(8, 8), bounces=b, denoise=True),
                  'conv': rl.render(pose, Km, 64, 64, samples=(512, 512), bounces=b),
                  'conv_dn': rl.render(pose, Km, 64, 64, samples=(512, 512), bounces=b, denoise=True)}
    return out


def _rmse(a, b, hit):
    return float(((a[hit] - b[hit]).double() ** 2).mean().sqrt())


@pytest.mark.parametrize('bounces', [0, 1])
def test_a_denoised_render_lies_closer_to_the_converged_one(views, bounces):
    """RMSE to the 512+512 render over the covered pixels: strictly lower with denoise=True than without, for rgb_lin and, with one bounce,
    for indirect_lin; denoising the converged render moves it by less than the 8+8 render's RMSE"""
    r = views[bounces]
    hit = r['conv']['alpha'][..., 0] > 0
    assert 1500 < int(hit.sum()) < 64 * 64
    for key in ('rgb_lin',) + (('indirect_lin',) if bounces else ()):
        noisy, dn = _rmse(r['noisy'][key], r['conv'][key], hit), _rmse(r['noisy_dn'][key], r['conv'][key], hit)
        moved = _rmse(r['conv_dn'][key], r['conv'][key], hit)
        print(f'bounces {bounces} {key}: rmse to converged 8+8 {noisy:.4e}, 8+8 denoised {dn:.4e} (x{noisy / dn:.2f}); '
              f'denoising the converged render moves it {moved:.4e} ({moved / noisy:.3f} of the 8+8 rmse)')
        assert dn < noisy and moved < noisy
    assert float(r['conv']['indirect_lin'][hit].mean()) > 0 if bounces else 'indirect_lin' not in r['noisy_dn']


@pytest.mark.parametrize('bounces', [0, 1])
def test_the_denoised_render_keeps_everything_but_the_light(views, bounces):
    r = views[bounces]
    plain, dn = r['noisy'], r['noisy_dn']
    assert set(dn) == set(plain) | {'rgb_lin_raw'}
    for k in ('alpha', 'depth', 'albedo', 'metallic', 'roughness', 'normal'):
        assert torch.equal(dn[k], plain[k]), k
    assert torch.equal(_bits(dn['rgb_lin_raw']), _bits(plain['rgb_lin']))             # the unfiltered sum: the plain render's bits
    assert not torch.equal(dn['rgb_lin'], plain['rgb_lin']) and bool(torch.isfinite(dn['rgb_lin']).all())
    miss = plain['alpha'][..., 0] == 0
    assert int(miss.sum()) > 0 and not dn['rgb_lin'][miss].any()


def test_denoise_none_is_the_call_without_the_argument(views):
    rl, pose, Km = views['rl'], views['pose'], views['K']
    for b in (0, 1):
        for arg in (None, False):
            same = rl.render(pose, Km, 64, 64, samples=(8, 8), bounces=b, denoise=arg)
            assert set(same) == set(views[b]['noisy'])
            for k, t in views[b]['noisy'].items():
                assert torch.equal(_bits(same[k]) if same[k].dtype == torch.float32 else same[k], _bits(t) if t.dtype == torch.float32 else t), k


def test_supersampling_filters_before_the_box_filter_and_keeps_alpha(views):
    rl, pose, Km = views['rl'], views['pose'], views['K']
    bg = np.asarray([0.1, 0.2, 0.3], np.float32)
    plain = rl.render(pose, Km, 32, 32, samples=(8, 8), ssaa=2, bounces=1, background=bg)
    dn = rl.render(pose, Km, 32, 32, samples=(8, 8), ssaa=2, bounces=1, background=bg, denoise={'iterations': 3, 'sigma_l': 2.0})
    assert torch.equal(_bits(dn['alpha']), _bits(plain['alpha'])) and tuple(dn['rgb_lin'].shape) == (32, 32, 3)
    assert torch.equal(_bits(dn['rgb_lin_raw']), _bits(plain['rgb_lin'])) and bool(torch.isfinite(dn['rgb_lin']).all())
    assert not torch.equal(dn['rgb_lin'], plain['rgb_lin']) and not torch.equal(dn['indirect_lin'], plain['indirect_lin'])
    with pytest.raises(ValueError, match='unknown parameters'):
        rl.render(pose, Km, 8, 8, denoise={'sigma': 1.0})


def test_the_script_takes_denoise(views, tmp_path):
    """scripts/relight.py --denoise --denoise-iterations 3 --denoise-sigma 2 writes render(denoise={'iterations': 3, 'sigma_l': 2.0})'s
    pixels, and they are not the plain render's; the two options without --denoise are refused"""
    import importlib.util
    import os
    from nero_amd import relight as RL
    from nero_amd.envlight import write_hdr
    from nero_amd.mesh import write_ply
    from nero_amd.texture import read_png
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('relight_script', os.path.join(root, 'scripts', 'relight.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    rl = views['rl']
    write_ply(str(tmp_path / 'm.ply'), rl.verts.cpu().numpy(), rl.tris.int().cpu().numpy())
    os.makedirs(tmp_path / 'mat')
    mats = {'metallic': rl.mat5[:, 0:1].cpu().numpy(), 'roughness': rl.mat5[:, 1:2].cpu().numpy(), 'albedo': rl.mat5[:, 2:5].cpu().numpy()}
    for k, a in mats.items():
        np.save(tmp_path / 'mat' / f'{k}.npy', a)
    write_hdr(str(tmp_path / 'e.hdr'), rl.env.cpu().numpy())
    argv = ['--mesh', str(tmp_path / 'm.ply'), '--material', str(tmp_path / 'mat'), '--hdr', str(tmp_path / 'e.hdr'), '--name', 'orbit', '--out',
            str(tmp_path / 'out'), '--num', '1', '--width', '32', '--height', '32', '--samples', '8', '8', '--cam_dist', '2.6', '--elevation', '40']
    script.main(argv + ['--denoise', '--denoise-iterations', '3', '--denoise-sigma', '2'])
    img = read_png(str(tmp_path / 'out' / 'orbit' / '0.png'))
    again = RL.Relighter(rl.verts, rl.tris, mats, str(tmp_path / 'e.hdr'))               # (the map as the script reads it back: RGBE-rounded)
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(1, 0.0, 40.0, 2.6))[0]
    want = again.render(pose, RL.default_K(32, 32), 32, 32, samples=(8, 8), denoise={'iterations': 3, 'sigma_l': 2.0})['rgba8'].cpu().numpy()
    plain = again.render(pose, RL.default_K(32, 32), 32, 32, samples=(8, 8))['rgba8'].cpu().numpy()
    assert img.shape == (32, 32, 4) and np.array_equal(img, want) and not np.array_equal(img, plain) and np.array_equal(img[..., 3], plain[..., 3])
    for lone in (['--denoise-iterations', '3'], ['--denoise-sigma', '2']):
        with pytest.raises(SystemExit):
            script.main(argv + lone)
