"""GPU tier of the validation metrics (nero_amd/metrics.py, nero_amd/csrc/image_metrics.hip) against the numpy restatements of
tests/metrics_ref.py: the quantiser bit for bit, the sum of squared differences exactly, SSIM within 1e-12 and PSNR within 1e-10 dB of the
integer restatement, run-to-run and workspace independence, the metric classes with their panels, and ValidationEvaluator end to end on both
renderers.

Tolerances.  The window sums are exact integers on both sides; what differs between the kernel and ssim_int is a few float64 roundings per
window (1e-16 relative) and the order of a mean of at most 34 000 terms of magnitude <= 1: 1e-12 absolute leaves three orders of magnitude
over that.  PSNR is one float64 log10 of an exact ratio: 1e-10 dB.  Against the reference's float32 formula the library may be closer to the
exact value, not otherwise different: |psnr - psnr_ref32| <= |psnr_ref32 - psnr_exact| + 1e-9."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-12
PSNR_TOL = 1e-10


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()                     # (a copy: the shared references are read-only)


@functools.lru_cache(maxsize=None)
def reference(kind, h, w, c):
    """computed once per case and shared: (gt, pr, sse, psnr_exact, psnr_ref32, ssim, ssim per channel)"""
    gt, pr = R.make_pair(kind, h, w, c)
    ssim, per = R.ssim_int(gt, pr)
    for a in (gt, pr, per):
        a.setflags(write=False)
    return gt, pr, R.sse_exact(gt, pr), R.psnr_exact(gt, pr), float(R.psnr_ref32(gt, pr)), ssim, per


def raw_metrics(gt, pr, fill):
    """nero_img_metrics on a workspace of the caller's, every byte of it set to `fill` first -> (out [B,2], sse [B], ssim_c [B,C]) on the device"""
    from nero_amd import _lib as L
    from nero_amd import metrics as M
    B, h, w, c = gt.shape
    ws = torch.full((int(M._lib.nero_img_metrics_workspace_bytes(B, h, w, c)),), fill, dtype=torch.uint8, device='cuda')
    out = torch.empty((B, 2), dtype=torch.float64, device='cuda')
    sse = torch.empty(B, dtype=torch.int64, device='cuda')
    ssim_c = torch.empty((B, c), dtype=torch.float64, device='cuda')
    L.check(M._lib.nero_img_metrics(L.ptr(gt), L.ptr(pr), B, h, w, c, L.ptr(ws), L.ptr(sse), L.ptr(ssim_c), L.ptr(out), L.stream_ptr()))
    return out, sse, ssim_c


def same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def check_against_reference(out, sse, ssim_c, ref, what):
    _, _, sse_ref, psnr_ref, psnr32, ssim_ref, per_ref = ref
    out, sse, ssim_c = out.cpu().numpy(), sse.cpu().numpy(), ssim_c.cpu().numpy()
    print(f'{what}: sse {int(sse)} (ref {sse_ref}), psnr {out[0]!r} (exact {psnr_ref!r}, float32 formula {psnr32!r}), '
          f'ssim {out[1]!r} (ref {ssim_ref!r}), |ssim_c - ref| max {np.abs(ssim_c - per_ref).max():.3e}')
    assert int(sse) == sse_ref
    assert np.abs(ssim_c - per_ref).max() <= SSIM_TOL and abs(out[1] - ssim_ref) <= SSIM_TOL
    if sse_ref == 0:
        assert out[0] == np.inf and psnr_ref == np.inf and psnr32 == np.inf
    else:
        assert abs(out[0] - psnr_ref) <= PSNR_TOL
        assert abs(out[0] - psnr32) <= abs(psnr32 - psnr_ref) + 1e-9


# ---- the quantiser --------------------------------------------------------------------------------------------------------------------------
def quantise_values(n):
    """n float32 values: every k / 255 with its neighbours on both sides, the clamped ranges, and the values whose result the header defines;
    cut or filled up (seeded uniform noise over [-0.5, 1.5]) to n, the special values first where n is small"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1e30, -1e30, -1e-3, -1.0, 1.0000001, 1.5, 255.0, 0.5, 0.999999, 1e-45, -1e-45],
                       np.float32)
    grid = np.concatenate([special, k, np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf))]).astype(np.float32)
    if n <= len(grid):
        return grid[:n].copy()
    rg = np.random.default_rng(n)
    return np.concatenate([grid, rg.uniform(-0.5, 1.5, n - len(grid)).astype(np.float32)])


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 100003])
def test_quantise_bit_equal(n, offset):
    """offset 1: the same values one float further into a buffer, so that the pointer is not 16-byte aligned"""
    from nero_amd import metrics as M
    x = quantise_values(n)
    buf = torch.zeros(n + offset, dtype=torch.float32, device='cuda')
    buf[offset:] = dev(x)
    got = M.color_map_backward(buf[offset:]).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (n,)
    finite = np.isfinite(x)
    with np.errstate(invalid='ignore'):
        ref = R.color_map_backward(np.where(finite, x, 0))
    assert np.array_equal(got[finite], ref[finite])
    assert np.all(got[np.isnan(x)] == 0) and np.all(got[x == np.inf] == 255) and np.all(got[x == -np.inf] == 0)


def test_quantise_all_levels_and_shapes():
    from nero_amd import metrics as M
    x = quantise_values(17 + 3 * 256)
    got = M.color_map_backward(dev(x)).cpu().numpy()
    assert np.array_equal(got[17:], R.color_map_backward(x[17:]))                           # (the 17 special values come first)
    img = torch.rand(5, 7, 3, device='cuda')
    q = M.color_map_backward(img)
    assert q.shape == img.shape and np.array_equal(q.cpu().numpy(), R.color_map_backward(img.cpu().numpy()))
    assert M.color_map_backward(torch.empty(0, 3, device='cuda')).shape == (0, 3)            # n = 0: a no-op
    t = M.color_map_backward(img.permute(1, 0, 2))                                            # not contiguous: by logical layout
    assert np.array_equal(t.cpu().numpy(), R.color_map_backward(img.permute(1, 0, 2).cpu().numpy()))


# ---- SSIM / PSNR ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('c', R.CHANNELS)
@pytest.mark.parametrize('h,w', R.SHAPES)
def test_metrics_against_the_restatement(h, w, c, kind):
    ref = reference(kind, h, w, c)
    gt, pr = dev(ref[0])[None], dev(ref[1])[None]
    a = raw_metrics(gt, pr, 0x00)
    b = raw_metrics(gt, pr, 0xFF)                                   # what the workspace held before does not matter
    c2 = raw_metrics(gt, pr, 0x00)                                  # nor does the run
    check_against_reference(a[0][0], a[1][0], a[2][0], ref, f'{kind} {h}x{w}x{c}')
    for x, y, z in zip(a, b, c2):
        assert same_bits(x, y) and same_bits(x, z)


@pytest.mark.parametrize('h,w,c', [(41, 43, 3), (140, 270, 3), (43, 41, 1)])
def test_a_batch_gives_the_bits_of_single_calls(h, w, c):
    from nero_amd import metrics as M
    refs = [reference(kind, h, w, c) for kind in ('noise', 'shift8', 'white_black')]
    gt, pr = dev(np.stack([r[0] for r in refs])), dev(np.stack([r[1] for r in refs]))
    out, sse, ssim_c = M.image_metrics(gt, pr, details=True)
    assert out.shape == (3, 2) and out.dtype == torch.float64 and sse.shape == (3,) and ssim_c.shape == (3, c)
    for b, ref in enumerate(refs):
        o1, s1, c1 = M.image_metrics(gt[b], pr[b], details=True)
        assert same_bits(o1[0], out[b]) and same_bits(s1[0], sse[b]) and same_bits(c1[0], ssim_c[b])
        check_against_reference(out[b], sse[b], ssim_c[b], ref, f'batch image {b} {h}x{w}x{c}')


def test_float_images_and_the_scalar_functions():
    from nero_amd import metrics as M
    rg = np.random.default_rng(5)
    gt, pr = rg.uniform(-0.1, 1.1, (24, 20, 3)).astype(np.float32), rg.uniform(0, 1, (24, 20, 3)).astype(np.float32)
    qg, qp = R.color_map_backward(gt), R.color_map_backward(pr)
    out = M.image_metrics(dev(gt), dev(pr))
    assert same_bits(out, M.image_metrics(dev(qg), dev(qp))) and same_bits(out, M.image_metrics(dev(gt), dev(qp)))
    psnr, ssim = M.compute_psnr(dev(gt), dev(pr)), M.structural_similarity(dev(gt), dev(pr))
    assert isinstance(psnr, float) and isinstance(ssim, float)
    assert abs(psnr - R.psnr_exact(qg, qp)) <= PSNR_TOL and abs(ssim - R.ssim_int(qg, qp)[0]) <= SSIM_TOL
    assert M.compute_psnr(dev(qg), dev(qg)) == float('inf') and M.structural_similarity(dev(qg), dev(qg)) == 1.0


def test_non_contiguous_inputs_are_read_by_their_logical_layout():
    from nero_amd import metrics as M
    ref = reference('noise', 21, 21, 3)
    wide_g, wide_p = np.zeros((21, 30, 4), np.uint8) + 7, np.zeros((21, 30, 4), np.uint8) + 9
    wide_g[:, 4:25, :3], wide_p[:, 4:25, :3] = ref[0], ref[1]
    g, p = dev(wide_g)[:, 4:25, :3], dev(wide_p)[:, 4:25, :3]
    assert not g.is_contiguous()
    out, sse, ssim_c = M.image_metrics(g, p, details=True)
    check_against_reference(out[0], sse[0], ssim_c[0], ref, 'a strided view')
    chw = dev(np.ascontiguousarray(ref[0].transpose(2, 0, 1))).permute(1, 2, 0)        # channels first in memory
    assert same_bits(M.image_metrics(chw, dev(ref[1])), out)


def test_device_side_argument_errors():
    from nero_amd import metrics as M
    z = torch.zeros(16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='GPU'):
        M.image_metrics(z.cuda(), z)
    with pytest.raises(ValueError, match='smaller than'):
        M.image_metrics(torch.zeros(10, 16, 3, device='cuda'), torch.zeros(10, 16, 3, device='cuda'))
    with pytest.raises(TypeError):
        M.image_metrics(z.cuda().double(), z.cuda().double())


# ---- the metric classes ---------------------------------------------------------------------------------------------------------------------
def panel_views(h, w, seed):
    rg = np.random.default_rng(seed)
    f = lambda c, flat=True: rg.uniform(-0.05, 1.05, (h * w, c) if flat else (h, w, c)).astype(np.float32)
    shape = {'gt_rgb': f(3, False), 'ray_rgb': f(3, False), 'normal': f(3), 'human_light': f(3), 'diffuse_albedo': f(3), 'diffuse_light': f(3),
             'diffuse_color': f(3), 'specular_albedo': f(3), 'specular_light': f(3), 'specular_color': f(3), 'specular_ref': f(3),
             'metallic': f(1), 'roughness': f(1), 'occ_prob': f(1), 'indirect_light': f(3), 'depth': f(1)}
    mat = {'rgb_gt': f(3, False), 'rgb_pr': f(3, False), 'albedo': f(3, False), 'metallic': f(1, False), 'roughness': f(1, False),
           'specular_light': f(3, False), 'specular_color': f(3, False), 'diffuse_light': f(3, False), 'diffuse_color': f(3, False)}
    return shape, mat


def q3(x, h, w):
    img = R.color_map_backward(x).reshape(h, w, -1)
    return np.repeat(img, 3, -1) if img.shape[-1] == 1 else img


def expected_shape_panel(d, h, w):
    q = lambda k: q3(d[k], h, w)
    rows = [R.concat_images_list(*[q(k) for k in ('gt_rgb', 'ray_rgb', 'normal', 'human_light') if k in d])]
    from nero_amd.metrics import MATERIAL_KEYS
    mats = [q(k) for k in MATERIAL_KEYS if k in d]
    rows += [R.concat_images_list(*r) for r in (mats[0:3], mats[3:7], mats[7:]) if r]
    return R.concat_images_list(*rows, vert=True)


def expected_material_panel(d, h, w):
    q = lambda k: q3(d[k], h, w)
    imgs = [q(k) for k in ('rgb_gt', 'rgb_pr', 'albedo', 'metallic', 'roughness', 'specular_light', 'specular_color', 'diffuse_light',
                           'diffuse_color') if k in d]
    return R.concat_images_list(*[R.concat_images_list(*r) for r in (imgs[:5], imgs[5:]) if r], vert=True)


def check_scores(res, gt, pr):
    qg, qp = R.color_map_backward(gt), R.color_map_backward(pr)
    assert set(res) == {'psnr', 'ssim'}
    for k in res:
        assert isinstance(res[k], np.ndarray) and res[k].shape == (1,) and res[k].dtype == np.float64
    assert abs(res['psnr'][0] - R.psnr_exact(qg, qp)) <= PSNR_TOL
    assert abs(res['ssim'][0] - R.ssim_int(qg, qp)[0]) <= SSIM_TOL


def test_metric_classes_scores_and_panels(tmp_path):
    from nero_amd import metrics as M
    from nero_amd.texture import read_png
    h, w = 24, 20
    shape, mat = panel_views(h, w, 11)
    to_dev = lambda d: {k: dev(v) for k, v in d.items()}
    for name, cls, d, gt_key, pr_key, expect in (('shape', M.ShapeRenderMetrics, shape, 'gt_rgb', 'ray_rgb', expected_shape_panel),
                                                 ('mat', M.MaterialRenderMetrics, mat, 'rgb_gt', 'rgb_pr', expected_material_panel)):
        metric = cls({'vis_dir': str(tmp_path / 'vis'), 'vis_format': 'png'})
        res = metric(to_dev(d), {}, 300, data_index=2, model_name=f'{name}-val')
        check_scores(res, d[gt_key], d[pr_key])
        path = tmp_path / 'vis' / f'{name}-val' / '300-index-2.png'
        assert path.exists()
        assert np.array_equal(read_png(str(path)), expect(d, h, w))
        # absent keys are skipped and an empty row is dropped
        few = {k: v for k, v in d.items() if k in (gt_key, pr_key, 'normal', 'metallic', 'occ_prob', 'albedo')}
        res2 = metric(to_dev(few), {}, 301, data_index=0, model_name=f'{name}-val')
        assert res2['psnr'][0] == res['psnr'][0] and res2['ssim'][0] == res['ssim'][0]
        assert np.array_equal(read_png(str(tmp_path / 'vis' / f'{name}-val' / '301-index-0.png')), expect(few, h, w))
        # write_vis = False writes nothing
        quiet = cls({'vis_dir': str(tmp_path / 'quiet'), 'write_vis': False})
        res3 = quiet(to_dev(d), {}, 300, data_index=2, model_name=f'{name}-val')
        assert res3['psnr'][0] == res['psnr'][0] and not (tmp_path / 'quiet').exists()
    assert M.name2metrics == {'shape_render': M.ShapeRenderMetrics, 'mat_render': M.MaterialRenderMetrics}


def test_jpeg_panel_when_pil_is_importable(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from nero_amd import metrics as M
    h, w = 24, 20
    shape, _ = panel_views(h, w, 12)
    metric = M.ShapeRenderMetrics({'vis_dir': str(tmp_path)})
    assert metric.vis_format == 'jpg'
    metric({k: dev(v) for k, v in shape.items()}, {}, 5, data_index=0, model_name='m')
    img = np.asarray(Image.open(str(tmp_path / 'm' / '5-index-0.jpg')))
    assert img.shape == expected_shape_panel(shape, h, w).shape


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
class Capture:
    """a metric that keeps the outputs it is shown and reports nothing"""

    def __init__(self):
        self.outputs = []

    def __call__(self, outputs, data, step, **kwargs):
        self.outputs.append({k: v.detach().cpu().numpy() for k, v in outputs.items() if torch.is_tensor(v)})
        return {}


def test_validation_evaluator_with_the_shape_renderer(tmp_path):
    """the FakeDB set-up of tests/test_shape_render.py::test_train_eval_train_sequence_with_several_training_images, validated on two views"""
    from nero_amd import metrics as M
    from nero_amd.renderer import NeROShapeRenderer
    from nero_amd.synthetic import look_at_pose
    from nero_amd.texture import read_png

    class FakeDB:
        def __init__(self):
            rg = np.random.default_rng(0)
            self.imgs = rg.uniform(0, 1, (4, 32, 40, 3)).astype(np.float32)
            self.K = np.array([[40., 0, 20], [0, 40., 16], [0, 0, 1]], np.float32)
            self.poses = [look_at_pose(np.array(c, dtype=np.float64)) for c in ([3, 0, 0.5], [0, 3, 1.0], [-2, -2, 1.5], [2, -2, 0.7])]
        def get_img_ids(self): return [0, 1, 2, 3]
        def get_image(self, i): return self.imgs[i]
        def get_K(self, i): return self.K
        def get_pose(self, i): return self.poses[i]

    torch.manual_seed(1)
    net = NeROShapeRenderer({'train_ray_num': 256, 'test_ray_num': 100, 'n_samples': 16, 'n_importance': 16, 'n_bg_samples': 8,
                             'shader_config': {'human_light': True}, 'downsample_ratio': 0.5}, training=False).cuda()
    db = FakeDB()
    net._init_dataset(db)
    views = [0, 1]                                                  # a database object validates on its first view only: take two
    net.test_ids = views
    net.test_imgs_info = {'imgs': torch.from_numpy(db.imgs[views]), 'Ks': torch.from_numpy(np.stack([db.K for _ in views])),
                          'poses': torch.from_numpy(np.stack([db.poses[i] for i in views]).astype(np.float32))}
    spy = Capture()
    metric = M.name2metrics['shape_render']({'vis_dir': str(tmp_path), 'vis_format': 'png'})
    ev = M.ValidationEvaluator({'key_metric_name': 'psnr'})
    results, key = ev(net, [spy, metric], [{'index': i} for i in range(len(views))], 25000, 'fake', val_set_name='val')
    assert results['ssim'].shape == (2,) and np.isfinite(results['ssim']).all()
    assert np.isfinite(key) and key == results['psnr']
    per_view = []
    for i, out in enumerate(spy.outputs):
        assert out['ray_rgb'].shape == (16, 20, 3) and out['gt_rgb'].shape == (16, 20, 3)
        qg, qp = R.color_map_backward(out['gt_rgb']), R.color_map_backward(out['ray_rgb'])
        per_view.append(R.psnr_exact(qg, qp))
        assert abs(results['ssim'][i] - R.ssim_int(qg, qp)[0]) <= SSIM_TOL
        panel = read_png(str(tmp_path / 'fake-val' / f'25000-index-{i}.png'))
        assert np.array_equal(panel, expected_shape_panel(out, 16, 20))
        assert 'human_light' in out and panel.shape[1] >= 4 * 20
    assert abs(key - np.mean(per_view)) <= PSNR_TOL
    assert sorted(os.listdir(tmp_path / 'fake-val')) == ['25000-index-0.png', '25000-index-1.png']


def test_validation_evaluator_with_the_material_renderer(tmp_path):
    """the icosphere set-up of tests/test_material_render.py::test_material_trainer_entry_point_and_pretrace, validated on its first view"""
    from nero_amd import metrics as M
    from nero_amd.renderer import NeROMaterialRenderer
    from nero_amd.synthetic import icosphere, look_at_pose
    from nero_amd.texture import read_png
    v, f = icosphere(4, 0.5, 0.15)
    f = np.ascontiguousarray(f[:, ::-1])
    torch.manual_seed(0)
    net = NeROMaterialRenderer({'shader_cfg': dict(diffuse_sample_num=32, specular_sample_num=16, human_lights=True,
                                                   outer_light_version='sphere_direction'),
                                'database_name': 'real/x', 'train_ray_num': 128}, mesh=(v, f)).cuda()
    rg = np.random.default_rng(0)
    imgs = torch.from_numpy(rg.uniform(0, 1, (2, 48, 48, 3)).astype(np.float32))
    K = torch.tensor([[60., 0, 24], [0, 60., 24], [0, 0, 1]]).repeat(2, 1, 1)
    poses = torch.from_numpy(np.stack([look_at_pose(np.array(c, dtype=np.float64)) for c in ([2.5, 0, 0.5], [0, 2.5, 1.0])], 0))
    net.set_ray_pool(imgs, K, poses)
    spy = Capture()
    metric = M.name2metrics['mat_render']({'vis_dir': str(tmp_path), 'vis_format': 'png'})
    results, key = M.ValidationEvaluator({'key_metric_name': 'psnr'})(net, [spy, metric], [{'index': 0}], 100, 'mat')
    out = spy.outputs[0]
    assert out['rgb_pr'].shape == (48, 48, 3)
    qg, qp = R.color_map_backward(out['rgb_gt']), R.color_map_backward(out['rgb_pr'])
    assert np.isfinite(key) and abs(key - R.psnr_exact(qg, qp)) <= PSNR_TOL
    assert results['ssim'].shape == (1,) and abs(results['ssim'][0] - R.ssim_int(qg, qp)[0]) <= SSIM_TOL
    assert np.array_equal(read_png(str(tmp_path / 'mat' / '100-index-0.png')), expected_material_panel(out, 48, 48))


def test_eval_images_command_line(tmp_path, capsys):
    """scripts/eval_images.py in this process: two files, then two directories paired by name, with --json"""
    import importlib.util
    import json
    from nero_amd.texture import write_png
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('eval_images', os.path.join(root, 'scripts', 'eval_images.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    refs = {'a.png': reference('shift8', 41, 43, 3), 'b.png': reference('noise', 21, 21, 1)}
    for d in ('pr', 'gt'):
        os.makedirs(tmp_path / d)
    for name, ref in refs.items():
        write_png(str(tmp_path / 'gt' / name), ref[0] if ref[0].shape[-1] == 3 else ref[0][..., 0])
        write_png(str(tmp_path / 'pr' / name), ref[1] if ref[1].shape[-1] == 3 else ref[1][..., 0])
    write_png(str(tmp_path / 'pr' / 'only_here.png'), refs['b.png'][1][..., 0])
    rows, mean = cli.main(['--pr', str(tmp_path / 'pr' / 'a.png'), '--gt', str(tmp_path / 'gt' / 'a.png')])
    assert len(rows) == 1 and abs(rows[0]['psnr'] - refs['a.png'][3]) <= PSNR_TOL and abs(rows[0]['ssim'] - refs['a.png'][5]) <= SSIM_TOL
    rows, mean = cli.main(['--pr', str(tmp_path / 'pr'), '--gt', str(tmp_path / 'gt'), '--json', str(tmp_path / 'scores.json')])
    assert [r['name'] for r in rows] == ['a.png', 'b.png']
    for r in rows:
        assert abs(r['psnr'] - refs[r['name']][3]) <= PSNR_TOL and abs(r['ssim'] - refs[r['name']][5]) <= SSIM_TOL
    assert abs(mean['psnr'] - np.mean([refs[n][3] for n in refs])) <= PSNR_TOL and mean['pairs'] == 2
    saved = json.load(open(tmp_path / 'scores.json'))
    assert saved['mean'] == mean and saved['pairs'] == rows
    out = capsys.readouterr()
    assert 'mean ' in out.out and 'only_here.png' in out.err
