"""CPU tier of the denoiser (include/nero_hip_denoise.h, nero_amd/csrc/denoise.hip, nero_amd/denoise.py): the restatement
(tests/denoise_ref.py) on an analytic scene -- it lowers the noise, barely moves a clean picture, leaves uncovered pixels alone --, the
entry points' refusals before any device call, and the tile and grid arithmetic as a stand-alone program under the sanitizers.  The
header's binding: tests/test_binding_cpu.py."""
import numpy as np
import pytest

from tests import denoise_ref as DR
from tests.helpers import run_host_program

ERR_ARG = -1
PARAMS = dict(iterations=5, sigma_l=4.0, normal_pow2=6, sigma_p=0.05)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def scene():
    """the sphere over the plane at 40 x 48, 50 % multiplicative noise, seed 1, filtered once in float64: noisy and clean"""
    sc = DR.sphere_over_plane(40, 48, noise=0.5, seed=1)
    run = lambda rgb: DR.denoise(rgb, sc['pos'], sc['normal'], sc['valid'], 40, 48, dtype=np.float64, **PARAMS)
    sc['filtered'], sc['var'] = run(sc['noisy'])
    sc['clean_filtered'], _ = run(sc['clean'])
    return sc


# ---- 1. the restatement on the analytic scene -----------------------------------------------------------------------------------------------
def test_the_filter_lowers_the_noise(scene):
    """RMSE against the clean signal over the covered pixels falls by more than 2 (the prototype of the definition gave 3.95)"""
    v = scene['valid']
    before, after = DR.rmse(scene['noisy'], scene['clean'], v), DR.rmse(scene['filtered'], scene['clean'], v)
    print(f'rmse noisy {before:.4f} filtered {after:.4f} ratio {before / after:.2f}')
    assert before / after > 2.0


def test_the_filter_barely_moves_a_clean_picture(scene):
    """the bias: the filter applied to the clean signal moves it by less than a tenth of the noisy picture's RMSE (prototype: 0.004 against
    0.236)"""
    v = scene['valid']
    bias, noise = DR.rmse(scene['clean_filtered'], scene['clean'], v), DR.rmse(scene['noisy'], scene['clean'], v)
    print(f'bias {bias:.4f} noisy rmse {noise:.4f}')
    assert bias < noise / 10.0


def test_uncovered_pixels_are_unchanged(scene):
    u = ~scene['valid']
    assert u.sum() > 0
    assert np.array_equal(scene['filtered'][u], scene['noisy'][u].astype(np.float64))
    assert not scene['var'][u].any()
    sig = DR.pack_signal(scene['noisy'], var=np.full(len(u), 0.25))
    guide = DR.pack_guides(scene['pos'], scene['normal'], scene['valid'])
    for out in (DR.estimate_variance(guide, sig, 40, 48, dtype=np.float32), DR.atrous_pass(guide, sig, 40, 48, 2, dtype=np.float32)):
        assert np.array_equal(out[u].view(np.uint32), sig[u].view(np.uint32))            # all four columns, bit for bit
        assert not np.array_equal(out[~u], sig[~u])


def test_float32_restatement_stays_close_to_float64(scene):
    """the floor of the GPU parity tests: the restatement in float32 against itself in float64 (the prototype: 7e-7 to 9e-7 relative)"""
    f32, _ = DR.denoise(scene['noisy'], scene['pos'], scene['normal'], scene['valid'], 40, 48, dtype=np.float32, **PARAMS)
    assert f32.dtype == np.float32
    _, floor = DR.parity(f32, f32, scene['filtered'])
    print('float32 against float64', floor)
    assert 0 < floor < 1e-5


def test_a_constant_signal_and_perpendicular_halves_are_exact_in_the_restatement():
    """what the GPU tier asserts of the kernels holds in float32 arithmetic: a constant signal has variance exactly 0 (the moments are taken
    about the centre's luminance); perpendicular normals give a cross weight of exactly 0, so signals 0 and 1 on the two halves stay exactly
    0 and 1"""
    h, w = 9, 12
    sc = DR.sphere_over_plane(h, w, noise=0.0)
    valid = np.ones(h * w, bool)
    const = np.full((h * w, 3), 0.3, np.float32)
    guide = DR.pack_guides(sc['pos'], sc['normal'], valid)
    assert not DR.estimate_variance(guide, DR.pack_signal(const), h, w, dtype=np.float32)[:, 3].any()
    left = (np.arange(h * w) % w) < w // 2
    nrm = np.where(left[:, None], np.asarray([1.0, 0, 0], np.float32), np.asarray([0, 1.0, 0], np.float32))
    rgb = np.where(left[:, None], 0.0, 1.0).astype(np.float32).repeat(3, 1)
    out, var = DR.denoise(rgb, sc['pos'], nrm, valid, h, w, dtype=np.float32, **PARAMS)
    assert np.array_equal(out, rgb) and not var.any()


# ---- 2. the surface: refusals (the binding: tests/test_binding_cpu.py) ----------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device(L):
    lib = L.lib
    p, q = 4096, 8192                                                 # non-null pointers that are never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    inf, nan = float('inf'), float('nan')
    base = (('guide', p), ('G', 0), ('sig_in', p), ('h', 8), ('w', 8), ('step', 1), ('k', 6), ('sigma_l', 4.0), ('sigma_p', 0.05),
            ('sigma_g', 0.1), ('sig_out', q), ('stream', None))
    atrous = lambda **kw: lib.nero_denoise_atrous(*[kw.get(k, d) for k, d in base])
    variance = lambda **kw: lib.nero_denoise_variance(*[kw.get(k, d) for k, d in base if k not in ('step', 'sigma_l')])
    for name, call in (('nero_denoise_variance', variance), ('nero_denoise_atrous', atrous)):
        for h, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (2 ** 31, 1), (1, 2 ** 31), (65536, 32768), (46341, 46341), (2 ** 40, 2 ** 40), (2 ** 33 + 8, 1)):
            assert call(h=h, w=w) == ERR_ARG and 'h w below 2^31' in err() and err().startswith(name), (h, w)
        for G in (1, 8, -4, 3):
            assert call(G=G) == ERR_ARG and 'G must be 0 or 4' in err()
        for k in (-1, 11, 64):
            assert call(k=k) == ERR_ARG and 'k must be in [0, 10]' in err()
        for s in (0.0, -0.05, inf, -inf, nan):
            assert call(sigma_p=s) == ERR_ARG and 'sigma_p must be finite and positive' in err(), s
            assert call(G=4, sigma_g=s) == ERR_ARG and 'sigma_g must be finite and positive' in err(), s
            assert call(G=0, sigma_g=s, sig_out=p) == ERR_ARG and 'same buffer' in err()          # sigma_g is not read for G = 0: the next check speaks
        for arg in ('guide', 'sig_in', 'sig_out'):
            assert call(**{arg: None}) == ERR_ARG and 'null pointer' in err()
            assert call(**{arg: p + 4}) == ERR_ARG and '16-byte aligned' in err()
        assert call(sig_out=p) == ERR_ARG and 'sig_in and sig_out must not be the same buffer' in err()
    for step in (0, -1, 2 ** 20 + 1, 2 ** 31 - 1):
        assert atrous(step=step) == ERR_ARG and 'step must be in [1, 2^20]' in err()
    for s in (0.0, -4.0, inf, nan):
        assert atrous(sigma_l=s) == ERR_ARG and 'sigma_l must be finite and positive' in err()


def test_host_layer_refuses_bad_shapes_and_options():
    import torch
    from nero_amd import denoise as DN
    g, s = torch.zeros(12, 8), torch.zeros(12, 4)
    with pytest.raises(ValueError, match='expected for a 3 x 5 image'):
        DN.atrous_pass(g, s, 3, 5, 1)
    with pytest.raises(ValueError, match='expected for a 3 x 4 image'):
        DN.estimate_variance(torch.zeros(12, 9), s, 3, 4)
    with pytest.raises(ValueError, match='iterations'):
        DN.denoise_records(g, s, 3, 4, iterations=22)
    with pytest.raises(ValueError, match='unknown parameters'):
        DN.options({'sigma': 1.0}, 0.1)
    assert DN.options(None, 0.1) is None and DN.options(False, 0.1) is None
    assert DN.options(True, 0.25) == {**DN.DEFAULTS, 'sigma_p': 0.25}
    assert DN.options({'iterations': 3, 'sigma_p': 0.5}, 0.25) == {**DN.DEFAULTS, 'iterations': 3, 'sigma_p': 0.5}
    # the packers against the restatement's, bit for bit
    sc = DR.sphere_over_plane(6, 7)
    t = lambda k: torch.from_numpy(sc[k])
    for extra in (None, t('extra')):
        got = DN.pack_guides(t('pos'), t('normal'), t('valid'), extra).numpy()
        want = DR.pack_guides(sc['pos'], sc['normal'], sc['valid'], None if extra is None else sc['extra'])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(DN.pack_signal(t('noisy')).numpy().view(np.uint32), DR.pack_signal(sc['noisy']).view(np.uint32))


# ---- 3. tiles and grids ---------------------------------------------------------------------------------------------------------------------
def test_tile_and_grid_arithmetic_under_the_sanitizers(tmp_path):
    """nero_amd/csrc/denoise_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program): the tiles cover every
    shape of the GPU tier, 800 x 800, 1600 x 1600 and the limits; the grid stays within 2^20 workgroups; the argument checks hold at their
    edges"""
    lines = run_host_program(tmp_path, 'denoise_plan_main.cpp').splitlines()
    assert lines[-1] == 'bad 0'
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('S ')]
    assert len(rows) == 15
    for h, w, tx, ty, t, grid in rows:
        assert tx == -(-w // 32) and ty == -(-h // 8) and t == tx * ty and grid == min(t, 2 ** 20)
    lds = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('L ')]
    assert lds == [(1, 36 * 12, 36 * 12 * 48, 36 * 12 * 64), (2, 40 * 16, 40 * 16 * 48, 40 * 16 * 64), (0, 38 * 14, 38 * 14 * 48, 38 * 14 * 64)]
    assert max(r[-1] for r in lds) <= 65536
    got = {r[:2]: r[2:] for r in rows}
    assert got[(1, 1)] == (1, 1, 1, 1) and got[(9, 33)] == (2, 2, 4, 4) and got[(800, 800)] == (25, 100, 2500, 2500)
    assert got[(2 ** 31 - 1, 1)] == (1, 2 ** 28, 2 ** 28, 2 ** 20) and got[(1, 2 ** 31 - 1)] == (2 ** 26, 1, 2 ** 26, 2 ** 20)
