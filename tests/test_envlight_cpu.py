"""CPU tier of the environment-light export (nero_amd/envlight.py): the fixture tests/golden/env_light.npz (the unmodified reference's env_light,
scripts/gen_golden_envlight.py) -- its conditions, that the product's constructor path reproduces its weights, that the float64 truth of
tests/envlight_ref.py agrees with it -- and the Radiance RGBE definition and file format.  No GPU, no reference tree."""
import numpy as np
import pytest
import torch

from tests import envlight_ref as R
from tests.helpers import build_material_case


@pytest.fixture(scope='module')
def fixture():
    return R.load_fixture()


CASES = R.case_list()
NAMES = [n for n, _ in CASES]


def _model(meta, name):
    info = meta['cases'][name]
    net = build_material_case({'seed': meta['seed'], 'shader_cfg': info['shader_cfg']})
    return R.apply_recipe(net, info['recipe'])


def test_fixture_holds_the_cases_and_their_conditions(fixture):
    z, meta = fixture
    assert list(meta['cases']) == NAMES
    for name, case in CASES:
        info = meta['cases'][name]
        assert {k: info[k] for k in case} == case
        lin, gam = z['lin/' + name], z['gam/' + name]
        assert lin.dtype == np.float32 and lin.shape == (case['h'], case['w'], 3) and gam.shape == lin.shape
        nan = np.argwhere(np.isnan(lin).any(-1))
        if info['nan_pixel'] is None:
            assert len(nan) == 0 and not np.isnan(gam).any(), name                      # no NaN outside the recorded pixel
        else:
            assert info['nan_pixel'] == [8, 24] and nan.tolist() == [[8, 24]] and np.argwhere(np.isnan(gam).any(-1)).tolist() == [[8, 24]]
        fin = lin[~np.isnan(lin).any(-1)]
        ratio = float(fin.max() / fin.min())
        emax = info['shader_cfg'].get('light_exp_max', 5.0)
        clamped = float((fin >= np.float32(np.exp(emax)) * (1 - 1e-6)).mean())
        knee = float((fin <= R.SRGB_KNEE).mean())
        # a clamp case carries the weights of its plain case under a ceiling of exp(-0.7): its variation is the plain case's, its own
        # condition is the clamped share; the maps of a few pixels are in the fixture for their sizes
        if case['recipe'] != 'clamp' and case['h'] * case['w'] >= 512:
            assert ratio >= 1.03, (name, ratio)
        if case['recipe'] == 'gain':
            assert ratio >= 1.5, (name, ratio)
        if case['recipe'] == 'clamp':
            assert 0.1 <= clamped <= 0.9, (name, clamped)
            assert abs(float(fin.max()) / np.exp(-0.7) - 1) < 1e-6
        else:
            assert clamped == 0.0, (name, clamped)
        if case['recipe'] == 'toe':
            assert 0.1 <= knee <= 0.9, (name, knee)
        else:
            assert knee == 0.0, (name, knee)
    import os
    assert os.path.getsize(R.GOLD) < 1 << 20


@pytest.mark.parametrize('name', NAMES)
def test_the_product_constructor_reproduces_the_reference_weights(fixture, name):
    from oracle.golden_util import state_checksums
    z, meta = fixture
    net = _model(meta, name)
    sd = {k: v for k, v in net.state_dict().items() if k.startswith('shader_network.outer_light.')}
    keys = [k for k in z.files if k.startswith(f'ck/{name}/')]
    assert len(keys) == len(sd) == 12
    for k, v in state_checksums(sd).items():
        np.testing.assert_allclose(v, z[f'ck/{name}/{k}'], rtol=1e-6, atol=1e-9, err_msg=k)


@pytest.mark.parametrize('name', NAMES)
def test_the_float64_truth_agrees_with_the_reference(fixture, name, capsys):
    """the oracle on the float64 grid, evaluated in float32, against the reference's float32 panorama (the issue measured at most 7.1e-5), and
    the floor of the GPU tier: the reference's own distance from the float64 truth"""
    z, meta = fixture
    info = meta['cases'][name]
    net = _model(meta, name)
    grid = R.latlong_grid(info['h'], info['w'], info['is_real'])
    skip = info['nan_pixel']
    for gamma, key in ((False, 'lin/'), (True, 'gam/')):
        ref = z[key + name]
        t64 = R.truth_stage2(net.state_dict(), info['shader_cfg'], grid, gamma)
        t32 = R.truth_stage2(net.state_dict(), info['shader_cfg'], grid, gamma, torch.float32)
        assert np.isfinite(t64).all() and (t64 > 0).all()                                   # the z-axis pixel included: the finite limit
        agree, floor = R.rel_error(t32, ref, skip), R.rel_error(ref, t64, skip)
        with capsys.disabled():
            print(f'\n  {name} {"gamma" if gamma else "linear"}: oracle32 vs reference32 {agree:.2e}, floor (reference32 vs truth64) {floor:.2e}', end='')
        # both are float32 evaluations of the same function: each within the floor rule of the other's distance from the truth
        assert agree <= R.tolerance(max(floor, R.rel_error(t32, t64))), (name, gamma, agree, floor)


# ---- RGBE -------------------------------------------------------------------------------------------------------------------------------------
def _rgbe_inputs():
    rng = np.random.default_rng(5)
    mags = 10.0 ** rng.uniform(-38, 38, (400, 1))
    wide = (mags * rng.uniform(0, 1, (400, 3))).astype(np.float32)
    pow2 = np.stack([np.float32(2.0) ** np.arange(-120, 127, dtype=np.float32)] * 3, -1) * np.array([1, 0.5, 0.75], np.float32)
    special = np.array([[0, 0, 0], [1e-33, 0, 0], [9.9e-33, 9.9e-33, 0], [1e-32, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [255, 1, 0.99], [-1, 0.25, 0.1],
                        [-1, -2, -3], [0.3, -0.1, 1.9999999], [1e38, 1, 1e30]], np.float32)
    return np.concatenate([wide, pow2.astype(np.float32), special], 0)


def test_rgbe_restatement_decodes_to_within_one_step(fixture):
    z, _ = fixture
    x = np.concatenate([_rgbe_inputs()] + [np.nan_to_num(z['lin/' + n], nan=0.5).reshape(-1, 3) for n in NAMES[:4]], 0)
    b = R.rgbe_encode(x)
    ch = np.maximum(x, 0).astype(np.float64)
    v = ch.max(-1)
    zero = v < 1e-32
    assert (b[zero] == 0).all() and zero.sum() >= 4
    assert (b[~zero, 3] > 0).all()
    e = b[~zero, 3].astype(np.int64) - 128
    dec = R.rgbe_decode(b)[~zero]
    step = np.ldexp(1.0, e - 8)[:, None]
    assert ((dec <= ch[~zero]) & (ch[~zero] - dec < step)).all()                         # truncation: within 2^(e - 8) from below
    assert (step[:, 0] <= v[~zero] / 128).all()                                          # ... under 1 / 128 of the largest channel
    assert (b[~zero, :3].max(-1) >= 128).all()                                           # the largest channel's mantissa is in [0.5, 1)


def test_host_encoder_equals_the_restatement():
    from nero_amd import envlight as E
    x = _rgbe_inputs()
    assert np.array_equal(E.rgbe_encode_host(x), R.rgbe_encode(x))
    assert np.array_equal(E.rgbe_decode(R.rgbe_encode(x)).astype(np.float64), R.rgbe_decode(R.rgbe_encode(x)))


def test_write_hdr_then_read_hdr(tmp_path, fixture):
    from nero_amd import envlight as E
    z, _ = fixture
    img = z['lin/gain_direction_real']
    p = str(tmp_path / 'a.hdr')
    rgbe = E.write_hdr(p, img)
    raw = open(p, 'rb').read()
    head = b'#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 16 +X 32\n'
    assert raw.startswith(head) and len(raw) == len(head) + 16 * 32 * 4 and raw[len(head):] == rgbe.tobytes()
    assert np.array_equal(rgbe, R.rgbe_encode(img))
    back, bytes_back = E.read_hdr(p, return_rgbe=True)
    assert back.dtype == np.float32 and back.shape == (16, 32, 3) and np.array_equal(bytes_back, rgbe)
    assert np.array_equal(back.astype(np.float64), R.rgbe_decode(rgbe))
    assert np.abs(back - img).max() <= img.max() / 128
    E.write_hdr(p, torch.from_numpy(img[:1, :1].copy()))                                  # a host tensor, 1 x 1
    assert E.read_hdr(p).shape == (1, 1, 3)


def test_read_hdr_reads_run_length_scanlines(tmp_path):
    from nero_amd import envlight as E
    rng = np.random.default_rng(2)
    h, w = 3, 300
    rgbe = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    rgbe[0, 10:200] = rgbe[0, 10]                                                         # long runs (split at 127), short runs, literals
    rgbe[1, :, 3] = 129
    rgbe[2, 5:8, 0] = 7
    body = R.rle_scanline(rgbe[0]) + rgbe[1].tobytes() + R.rle_scanline(rgbe[2])          # a flat scanline between two encoded ones
    p = str(tmp_path / 'r.hdr')
    with open(p, 'wb') as fh:
        fh.write(b'#?RADIANCE\n# a comment\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y 3 +X 300\n' + body)
    assert len(R.rle_scanline(rgbe[0])) < 4 * w
    img, back = E.read_hdr(p, return_rgbe=True)
    assert np.array_equal(back, rgbe)
    assert np.array_equal(img.astype(np.float64), R.rgbe_decode(rgbe).astype(np.float32).astype(np.float64))
    hand = bytes([2, 2, 0, 8]) + bytes([128 + 8, 10]) + bytes([3, 1, 2, 3, 128 + 5, 9]) + bytes([8]) + bytes(range(8)) + bytes([128 + 8, 130])
    with open(p, 'wb') as fh:
        fh.write(b'#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 8\n' + hand)
    _, one = E.read_hdr(p, return_rgbe=True)
    want = np.stack([np.full(8, 10), np.array([1, 2, 3, 9, 9, 9, 9, 9]), np.arange(8), np.full(8, 130)], -1).astype(np.uint8)
    assert np.array_equal(one[0], want)
    with open(p, 'wb') as fh:
        fh.write(b'#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 8\n' + hand[:-3])
    with pytest.raises(ValueError):
        E.read_hdr(p)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -1e-3, 2.0 ** 127])
def test_write_hdr_refuses_what_rgbe_cannot_hold(tmp_path, bad):
    from nero_amd import envlight as E
    img = np.full((2, 3, 3), 0.5, np.float32)
    img[1, 2, 1] = bad
    p = tmp_path / 'bad.hdr'
    with pytest.raises(ValueError):
        E.write_hdr(str(p), img)
    with pytest.raises(ValueError):
        E.write_hdr(str(p), torch.from_numpy(img))
    assert not p.exists()                                                                 # nothing was written
    with pytest.raises(ValueError):
        E.write_hdr(str(p), np.zeros((4, 3), np.float32))
    E.write_hdr(str(p), np.full((1, 1, 3), np.float32(1.7e38)))                           # just below 2^127: fine
