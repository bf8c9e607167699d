"""GPU tier of the environment-light export: nero_amd/csrc/envlight.hip through its ABI and through NeROMaterialRenderer.env_light /
get_env_light and NeROShapeRenderer.env_light, against the float64 truth of tests/envlight_ref.py.

The rule (every comparison with a truth): error = the largest pointwise |p - t| / t; the product passes with error <= max(1e-4, 3 x floor), the
floor being the same error of a float32 evaluation that is not the code under test -- the reference's own panorama from
tests/golden/env_light.npz for Stage II, the oracle in float32 for get_env_light and Stage I.  Errors and floors go to the parity report
(tests.helpers.parity_report)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import envlight_ref as R
from tests.helpers import build_case_model, build_material_case, golden_mesh, load_golden, parity_report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.case_list()
NAMES = [n for n, _ in CASES]


@pytest.fixture(scope='module')
def E():
    from nero_amd import envlight
    return envlight


@pytest.fixture(scope='module')
def fixture():
    return R.load_fixture()


_MODELS = {}


def material_renderer(meta, name):
    """(NeROMaterialRenderer on the GPU carrying the case's weights, the CPU holder they came from), built once per case"""
    if name not in _MODELS:
        from nero_amd.renderer import NeROMaterialRenderer
        info = meta['cases'][name]
        ref = R.apply_recipe(build_material_case({'seed': meta['seed'], 'shader_cfg': info['shader_cfg']}), info['recipe'])
        net = NeROMaterialRenderer({'shader_cfg': info['shader_cfg'], 'database_name': 'real/case' if info['is_real'] else 'syn/case'},
                                   is_train=False, mesh=golden_mesh())
        net.load_state_dict(ref.state_dict())
        _MODELS[name] = (net.cuda().eval(), ref)
    return _MODELS[name]


# ---- directions through the ABI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('is_real', [False, True])
@pytest.mark.parametrize('h,w', [(16, 32), (17, 33), (1, 1), (1, 5), (3, 1), (2, 2), (67, 129)])
def test_directions_follow_the_float64_grid(E, h, w, is_real):
    """2e-6: float32 rounding of angles up to 3 pi / 2 (2.4e-7 each for the product and the sum) and of the linspace (3.7e-7), sinf / cosf
    and the final products -- a bound from the formats, for a float32 formulation; the kernel forms the angles in float64"""
    d = E.latlong_directions(h, w, is_real)
    assert d.dtype == torch.float32 and tuple(d.shape) == (h, w, 3) and d.is_cuda and d.is_contiguous()
    grid = R.latlong_grid(h, w, is_real)
    got = d.cpu().numpy().astype(np.float64)
    assert np.abs(got - grid).max() <= 2e-6
    assert np.abs(np.linalg.norm(got, axis=-1) - 1).max() <= 1e-6
    assert torch.equal(d[:, 0], d[:, -1])                                                # az = 3 pi / 2 and -pi / 2: the same direction
    up = 2 if is_real else 1
    pole = np.zeros(3)
    pole[up] = 1.0
    assert np.abs(got[0] - pole).max() <= 1e-7                                           # row 0 at the pole el = +pi / 2
    if h > 1:
        assert np.abs(got[-1] + pole).max() <= 1e-7


def test_encode_window_starts_mid_row_and_writes_whole_rows(E):
    """nero_env_encode on pixels first .. first + n - 1 of a 17 x 33 panorama with first mid-row and n no multiple of 64: the directions and
    the encodings equal the rows of the full call bit for bit, the padding rows are zero, sphere doubles the 72 columns, nothing is written
    beyond row_pad(n) rows or n directions"""
    from nero_amd import _lib as L
    h, w, first, n = 17, 33, 40, 150
    rp = (n + 63) // 64 * 64
    full = torch.empty((640, 72), device='cuda')
    fdirs = torch.empty((h * w, 3), device='cuda')
    L.check(L.lib.nero_env_encode(h, w, 0, h * w, 0, 0, 0.0, L.ptr(full), L.ptr(fdirs), L.stream_ptr()))
    for sphere in (0, 1):
        ld = 144 if sphere else 72
        X = torch.full((rp + 64, ld), 7.0, device='cuda')
        dirs = torch.full((n + 8, 3), 7.0, device='cuda')
        L.check(L.lib.nero_env_encode(h, w, first, n, 0, sphere, 0.0, L.ptr(X), L.ptr(dirs), L.stream_ptr()))
        assert torch.equal(dirs[:n], fdirs[first:first + n]) and bool((dirs[n:] == 7.0).all())
        assert torch.equal(X[:n, :72], full[first:first + n])
        if sphere:
            assert torch.equal(X[:n, 72:], X[:n, :72])
        assert bool((X[n:rp] == 0).all()) and bool((X[rp:] == 7.0).all())
    assert torch.equal(fdirs.view(h, w, 3), E.latlong_directions(h, w, False))
    # the encoding is the IDE: against the oracle's in float64 on the same directions, within 3 x what the oracle's own float32 evaluation
    # is off by (degree-16 polynomials with alternating coefficients of ~1e5 cancel in float32 whoever evaluates them)
    from oracle import nero_oracle as O
    enc = O.ide(fdirs.double().cpu(), 0.0).numpy()
    floor = float(np.abs(O.ide(fdirs.cpu(), 0.0).numpy() - enc).max())
    err = float(np.abs(full[:h * w].cpu().numpy() - enc).max())
    print(f'IDE through nero_env_encode: error {err:.3e}, float32 oracle {floor:.3e}')
    assert np.isfinite(full[:h * w].cpu().numpy()).all() and err <= max(1e-6, 3 * floor)
    for bad in ((0, 5, 0, 0), (5, 16385, 0, 1), (4, 4, 10, 7), (4, 4, -1, 2)):
        with pytest.raises(L.NeroHipError, match='libnero_hip error -1'):
            L.check(L.lib.nero_env_encode(bad[0], bad[1], bad[2], bad[3], 0, 0, 0.0, L.ptr(full), None, L.stream_ptr()))


# ---- the fixture's cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_env_light_meets_the_reference_floor_rule(fixture, name):
    z, meta = fixture
    info = meta['cases'][name]
    net, ref = material_renderer(meta, name)
    h, w = info['h'], info['w']
    grid = R.latlong_grid(h, w, info['is_real'])
    report = {}
    for gamma, key in ((False, 'lin'), (True, 'gam')):
        got = net.env_light(h, w, gamma=gamma)
        assert got.dtype == torch.float32 and tuple(got.shape) == (h, w, 3) and got.is_cuda and got.is_contiguous()
        p = got.cpu().numpy()
        truth = R.truth_stage2(ref.state_dict(), info['shader_cfg'], grid, gamma)
        floor = R.rel_error(z[f'{key}/{name}'], truth, info['nan_pixel'])
        err = R.rel_error(p, truth)                                                      # every pixel, the reference's NaN pixel included
        report[key] = dict(error=err, floor=floor, tolerance=R.tolerance(floor))
        print(f'{name} {key}: error {err:.3e}, floor {floor:.3e}, tolerance {R.tolerance(floor):.3e}')
        assert np.isfinite(p).all(), (name, key)
        assert err <= R.tolerance(floor), (name, key, err, floor)
        if info['recipe'] == 'clamp' and not gamma:
            assert 0.1 <= float((p >= np.exp(-0.7) * (1 - 1e-6)).mean()) <= 0.9 and float(p.max()) <= np.exp(-0.7) * (1 + 1e-6)
        if info['recipe'] == 'toe' and gamma:
            assert 0.1 <= float((p <= 323 / 25 * R.SRGB_KNEE).mean()) <= 0.9                 # both branches of linear_to_srgb are taken
    parity_report(f'test_envlight_gpu::{name}', size=[h, w], **report)


def test_get_env_light_meets_the_oracle_floor_rule(fixture):
    z, meta = fixture
    for name in ('gain_direction_syn', 'plain_sphere_direction_real', 'clamp_direction_real'):
        info = meta['cases'][name]
        net, ref = material_renderer(meta, name)
        got = net.get_env_light()
        assert got.dtype == torch.float32 and tuple(got.shape) == (8192, 3) and got.is_cuda
        pts = ref.shader_network.light_pts.double().numpy()
        truth = R.truth_stage2(ref.state_dict(), info['shader_cfg'], pts, False)
        floor = R.rel_error(R.truth_stage2(ref.state_dict(), info['shader_cfg'], pts, False, torch.float32), truth)
        err = R.rel_error(got.cpu().numpy(), truth)
        print(f'get_env_light {name}: error {err:.3e}, floor {floor:.3e}')
        parity_report(f'test_envlight_gpu::get_env_light::{name}', error=err, floor=floor, tolerance=R.tolerance(floor))
        assert err <= R.tolerance(floor), (name, err, floor)
        assert torch.equal(got, net.get_env_light())


# ---- Stage I ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('golden', ['bell_s25000', 'bell_sphdir'])
def test_stage1_env_light_meets_the_oracle_floor_rule(golden):
    """AppShadingNetwork.outer_light on IDE(d, roughness): sphere_direction off (bell) and on (bell_sphdir), roughness 0, 0.25 and 1, linear and
    gamma; light_exp_max is 0, so the light is clamped at 1.0 -- the second round moves the last bias so that about half of the map clamps"""
    _, meta = load_golden(golden)
    ref = build_case_model(meta)
    net = build_case_model(meta).cuda().eval()
    sphere = bool(meta['cfg'].get('shader_config', {}).get('sphere_direction', False))
    assert sphere == (golden == 'bell_sphdir')
    exp_max = net.color_network.cfg['light_exp_max']
    assert exp_max == 0.0
    h, w = 16, 32
    grid = R.latlong_grid(h, w, False)                                                   # database_name of the golden cases is synthetic
    assert not str(net.cfg['database_name']).startswith('real')
    _, raw0 = R.truth_stage1(ref.state_dict(), sphere, exp_max, grid, 0.0, False)
    shift = -float(np.median(raw0))
    for bias_shift in (0.0, shift):
        if bias_shift:
            with torch.no_grad():
                net.color_network.outer_light[6].bias.add_(bias_shift)
        for rough in (0.0, 0.25, 1.0):
            for gamma in (False, True):
                truth, raw = R.truth_stage1(ref.state_dict(), sphere, exp_max, grid, rough, gamma, bias_shift=bias_shift)
                t32, _ = R.truth_stage1(ref.state_dict(), sphere, exp_max, grid, rough, gamma, torch.float32, bias_shift=bias_shift)
                floor = R.rel_error(t32, truth)
                got = net.env_light(h, w, gamma=gamma, roughness=rough)
                assert got.dtype == torch.float32 and tuple(got.shape) == (h, w, 3) and got.is_contiguous()
                err = R.rel_error(got.cpu().numpy(), truth)
                clamped = float((raw > exp_max).mean())
                print(f'{golden} shift {bias_shift:.3f} roughness {rough} gamma {gamma}: error {err:.3e}, floor {floor:.3e}, clamped {clamped:.2f}')
                parity_report(f'test_envlight_gpu::stage1::{golden}::shift{int(bool(bias_shift))}::r{rough}::g{int(gamma)}', error=err, floor=floor,
                              tolerance=R.tolerance(floor), clamped_share=clamped)
                assert err <= R.tolerance(floor), (golden, bias_shift, rough, gamma, err, floor)
                if bias_shift and rough == 0.0:
                    assert 0.1 <= clamped <= 0.9
                    if not gamma:
                        assert float(got.max()) == 1.0 and 0.1 <= float((got == 1.0).float().mean()) <= 0.9
    lin0 = net.env_light(h, w, gamma=False, roughness=0.0)
    lin1 = net.env_light(h, w, gamma=False, roughness=1.0)
    assert not torch.equal(lin0, lin1)                                                   # the roughness reaches the encoding


# ---- bit identity -------------------------------------------------------------------------------------------------------------------------------
def test_env_light_is_bit_identical_run_to_run_and_for_every_chunking(fixture):
    z, meta = fixture
    for name in ('zaxis_direction_syn', 'gain_sphere_direction_real'):
        net, _ = material_renderer(meta, name)
        h, w = 17, 33                                                                    # 561 rows: chunks of 100 and 64 end ragged and cross the 64-row tile
        base = net.env_light(h, w, gamma=True)
        assert base.dtype == torch.float32 and tuple(base.shape) == (h, w, 3) and base.is_contiguous() and base.is_cuda
        assert torch.equal(base, net.env_light(h, w, gamma=True))
        for chunk in (561, 100, 64, 1):
            assert torch.equal(base, net.env_light(h, w, gamma=True, chunk=chunk)), (name, chunk)
        assert torch.equal(base, net.env_light(h, w, gamma=True, chunk=10 ** 9))
        with pytest.raises(ValueError):
            net.env_light(h, w, chunk=0)
        with pytest.raises(ValueError):
            net.env_light(0, w)


# ---- RGBE ---------------------------------------------------------------------------------------------------------------------------------------
def test_rgbe_kernel_equals_the_numpy_restatement(E, fixture):
    z, _ = fixture
    rng = np.random.default_rng(11)
    wide = ((10.0 ** rng.uniform(-38, 38, (3000, 1))) * rng.uniform(0, 1, (3000, 3))).astype(np.float32)
    pow2 = (np.stack([np.float32(2.0) ** np.arange(-126, 127, dtype=np.float32)] * 3, -1) * np.array([1, 0.5, 0.75], np.float32)).astype(np.float32)
    special = np.array([[0, 0, 0], [1e-33, 0, 0], [9.9e-33, 9.9e-33, 0], [1e-32, 0, 0], [1.0000001e-32, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [255, 1, 0.99],
                        [-1, 0.25, 0.1], [-1, -2, -3], [0.3, -0.1, 1.9999999], [1e38, 1, 1e30], [1e-38, 1e-38, 1e-38], [0.99999994, 0.5, 0.25]],
                       np.float32)
    panos = [np.nan_to_num(z[f'{k}/{n}'], nan=0.5).reshape(-1, 3) for n in NAMES for k in ('lin', 'gam')]
    x = np.concatenate([wide, pow2, special] + panos, 0)
    got = E.rgbe_encode(torch.from_numpy(x).cuda())
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(x), 4)
    want = R.rgbe_encode(x)
    bad = np.nonzero((got.cpu().numpy() != want).any(-1))[0]
    assert len(bad) == 0, (len(bad), x[bad[:4]], got.cpu().numpy()[bad[:4]], want[bad[:4]])
    one = E.rgbe_encode(torch.tensor([[0.25, 1.5, 0.75]], device='cuda'))                  # n = 1
    assert one.cpu().numpy().tolist() == [[32, 192, 96, 129]]
    img = torch.from_numpy(z['lin/gain_direction_real']).cuda()
    assert tuple(E.rgbe_encode(img).shape) == (16, 32, 4)
    assert np.array_equal(E.rgbe_encode(img).cpu().numpy(), R.rgbe_encode(z['lin/gain_direction_real']))
    with pytest.raises(ValueError):
        E.rgbe_encode(torch.zeros(4, 4, device='cuda'))


# ---- command line -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', [2, 1])
def test_command_line_writes_what_the_methods_return(E, fixture, tmp_path, stage):
    from nero_amd.metrics import color_map_backward
    from nero_amd.texture import read_png
    z, meta = fixture
    if stage == 2:
        name = 'gain_direction_real'
        net, ref = material_renderer(meta, name)
        cfg = {'shader_cfg': meta['cases'][name]['shader_cfg'], 'database_name': 'real/case'}
        sd, extra, kw = ref.state_dict(), [], {}
    else:
        _, gm = load_golden('bell_sphdir')
        ref = build_case_model(gm)
        net = build_case_model(gm).cuda().eval()
        cfg, sd, extra, kw = gm['cfg'], ref.state_dict(), ['--roughness', '0.25'], {'roughness': 0.25}
    with open(tmp_path / 'cfg.json', 'w') as fh:
        json.dump(cfg, fh)
    torch.save({'network_state_dict': sd}, tmp_path / 'model.pth')
    out = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'extract_env_light.py'), '--cfg', str(tmp_path / 'cfg.json'), '--model', str(tmp_path / 'model.pth'),
           '--stage', str(stage), '--height', '8', '--width', '16', '--out', str(out)] + extra
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    rec = json.loads(res.stdout.strip().split('\n')[-1])
    assert rec['height'] == 8 and rec['width'] == 16 and rec['stage'] == stage
    lin, gam = net.env_light(8, 16, gamma=False, **kw), net.env_light(8, 16, gamma=True, **kw)
    img, rgbe = E.read_hdr(str(out / 'env_light.hdr'), return_rgbe=True)
    assert np.array_equal(rgbe, E.rgbe_encode(lin).cpu().numpy())
    assert np.array_equal(img, E.rgbe_decode(E.rgbe_encode(lin)))
    assert np.array_equal(read_png(str(out / 'env_light.png')), color_map_backward(gam).cpu().numpy())
