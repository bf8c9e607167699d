"""CPU tier of the validation metrics (nero_amd/metrics.py, nero_amd/csrc/image_metrics.hip): the exported C ABI, the two SSIM restatements of
tests/metrics_ref.py against each other and against closed forms, the panel glue on host tensors, ValidationEvaluator with stubs, and the
argument checks that must refuse before anything is launched.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('nero_img_quantize', 'nero_img_metrics_workspace_bytes', 'nero_img_metrics')
CASES = [(h, w, c, kind) for (h, w) in R.SHAPES for c in R.CHANNELS for kind in R.KINDS]


def test_symbols_are_exported_and_declared():
    from nero_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'nero_hip.h')).read()
    for name in SYMBOLS:
        assert hasattr(L.lib, name), name
        assert name + '(' in header, name
    assert 'NaN -> 0' in header                       # the cast numpy leaves undefined is defined by the header


def test_workspace_query_and_c_level_argument_errors():
    """NERO_ERR_ARG (-1) for every shape outside the limits, with null pointers: refused before any pointer is touched or kernel launched"""
    import ctypes as C
    from nero_amd import metrics as M
    lib = M._lib
    assert lib.nero_img_metrics_workspace_bytes(1, 11, 11, 1) >= 40
    assert lib.nero_img_metrics_workspace_bytes(3, 140, 270, 3) >= 3 * 5 * 9 * 40
    for B, h, w, c in ((1, 10, 11, 3), (1, 11, 10, 3), (1, 11, 11, 0), (1, 11, 11, 5), (0, 11, 11, 3), (65536, 11, 11, 3), (1, 16385, 11, 1),
                       (1, 11, 16385, 1)):
        assert lib.nero_img_metrics_workspace_bytes(B, h, w, c) == 0, (B, h, w, c)
        assert lib.nero_img_metrics(None, None, B, h, w, c, None, None, None, None, None) == -1, (B, h, w, c)
    assert lib.nero_img_metrics(None, None, 1, 11, 11, 3, None, None, None, None, None) == -1            # null pointers
    assert lib.nero_img_quantize(None, 0, None, None) == 0                                               # n = 0: a no-op
    assert lib.nero_img_quantize(None, -1, None, None) == -1
    assert lib.nero_img_quantize(None, 5, None, None) == -1


@pytest.mark.parametrize('h,w,c,kind', CASES)
def test_ssim_restatements_agree(h, w, c, kind):
    gt, pr = R.make_pair(kind, h, w, c)
    m_ref, per_ref = R.ssim_ref(gt, pr)
    m_int, per_int = R.ssim_int(gt, pr)
    assert np.abs(per_ref - per_int).max() <= 1e-13 and abs(m_ref - m_int) <= 1e-13, (np.abs(per_ref - per_int).max(), m_ref - m_int)


@pytest.mark.parametrize('h,w,c', [(11, 11, 1), (11, 13, 3), (43, 41, 3)])
def test_closed_forms(h, w, c):
    gt, pr = R.make_pair('same', h, w, c)
    for f in (R.ssim_ref, R.ssim_int):
        assert f(gt, pr)[0] == 1.0
    assert R.psnr_exact(gt, pr) == float('inf')
    gt, pr = R.make_pair('white_black', h, w, c)
    expect = R.C1 / (65025 + R.C1)
    assert abs(expect - 9.99900009999e-5) < 1e-15
    for f in (R.ssim_ref, R.ssim_int):
        assert abs(f(gt, pr)[0] - expect) <= 1e-15
    assert R.sse_exact(gt, pr) == 65025 * h * w * c and R.psnr_exact(gt, pr) == 0.0
    assert abs(R.psnr_ref32(gt, pr)) < 2e-3            # the float32 means of the reference's formula: up to 2e-3 dB off


def test_quantise_restatement():
    x = np.array([-1.0, -0.0, 0.0, 0.5 / 255, 1.0 / 255, 0.5, 254.999 / 255, 1.0, 2.0, 1e30, np.inf, -np.inf], np.float32)
    assert R.color_map_backward(x).tolist() == [0, 0, 0, 0, 1, 127, 254, 255, 255, 255, 255, 0]


def _img(rg, h, w, c=3):
    return rg.integers(0, 256, (h, w, c), dtype=np.uint8)


def test_concat_images_list_on_host_tensors():
    from nero_amd import metrics as M
    rg = np.random.default_rng(0)
    a, b, c = _img(rg, 12, 9), _img(rg, 7, 14), _img(rg, 15, 3)
    ta, tb, tc = (torch.from_numpy(x) for x in (a, b, c))
    for vert in (False, True):
        got = M.concat_images_list(ta, tb, tc, vert=vert)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), R.concat_images_list(a, b, c, vert=vert))
    row = M.concat_images_list(ta, tb)                             # the shorter image is padded with zeros at the bottom
    assert row.shape == (12, 23, 3) and int(row[7:, 9:].sum()) == 0 and np.array_equal(row[:7, 9:].numpy(), b)
    col = M.concat_images_list(ta, tb, vert=True)                  # the narrower one at the right
    assert col.shape == (19, 14, 3) and int(col[:12, 9:].sum()) == 0 and np.array_equal(col[:12, :9].numpy(), a)
    assert M.concat_images_list(ta) is ta
    with pytest.raises(ValueError):
        M.concat_images_list()
    with pytest.raises(TypeError):
        M.concat_images_list(ta.float(), tb)


def test_draw_materials_on_host_tensors():
    from nero_amd import metrics as M
    rg = np.random.default_rng(1)
    h, w = 6, 5
    data = {k: _img(rg, h, w, 1 if k in ('metallic', 'roughness', 'occ_prob') else 3) for k in M.MATERIAL_KEYS if k != 'specular_ref'}
    data['unrelated'] = _img(rg, h, w)
    rows = M.draw_materials({k: torch.from_numpy(v).reshape(h * w, -1) for k, v in data.items()}, h, w)      # flat, as render_image returns them
    three = lambda k: np.repeat(data[k], 3, -1) if data[k].shape[-1] == 1 else data[k]
    present = [three(k) for k in M.MATERIAL_KEYS if k in data]
    expect = [np.concatenate(present[0:3], 1), np.concatenate(present[3:7], 1), np.concatenate(present[7:], 1)]
    assert len(rows) == 3 and all(np.array_equal(r.numpy(), e) for r, e in zip(rows, expect))
    # absent keys are skipped, an empty row is dropped
    rows = M.draw_materials({'metallic': torch.from_numpy(data['metallic'])}, h, w)
    assert len(rows) == 1 and np.array_equal(rows[0].numpy(), three('metallic'))
    assert M.draw_materials({}, h, w) == []


def test_validation_evaluator_with_stubs():
    from nero_amd import metrics as M

    class Model:
        def __init__(self):
            self.seen, self.was_eval, self.grad_on = [], False, None
        def eval(self):
            self.was_eval = True
        def __call__(self, data):
            self.seen.append(dict(data))
            self.grad_on = torch.is_grad_enabled()
            return {'view': data['index']}

    calls = []
    def metric(outputs, data, step, **kw):
        calls.append((outputs['view'], data['index'], step, kw['data_index'], kw['model_name']))
        return {'psnr': np.asarray([20.0 + outputs['view']]), 'ssim': torch.tensor([0.5 * outputs['view']], dtype=torch.float64)}

    assert set(M.name2metrics) == {'shape_render', 'mat_render'} and set(M.name2key_metrics) == {'psnr'}
    ev = M.ValidationEvaluator({'key_metric_name': 'psnr'})
    model = Model()
    dataset = [{'index': 3}, {'index': 1}, {'index': 4}]
    results, key = ev(model, [metric], dataset, 700, 'run', val_set_name='val')
    assert model.was_eval and model.grad_on is False
    assert [d['index'] for d in model.seen] == [3, 1, 4] and all(d['eval'] is True and d['step'] == 700 for d in model.seen)
    assert 'eval' not in dataset[0]                                                   # the caller's dicts are left alone
    assert calls == [(3, 3, 700, 0, 'run-val'), (1, 1, 700, 1, 'run-val'), (4, 4, 700, 2, 'run-val')]
    assert np.array_equal(results['ssim'], [1.5, 0.5, 2.0]) and results['ssim'].dtype == np.float64
    assert key == pytest.approx((23.0 + 21.0 + 24.0) / 3) and results['psnr'] == key
    _, key = ev(model, [metric], [{'index': 0}], 1, 'run')
    assert calls[-1][-1] == 'run' and key == 20.0
    with pytest.raises(KeyError):
        M.ValidationEvaluator({'key_metric_name': 'nothing'})


def test_argument_errors_before_any_launch():
    """host tensors throughout: every refusal below happens before the device is looked at, so none of them can have launched anything"""
    from nero_amd import metrics as M
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    with pytest.raises(ValueError, match='smaller than'):
        M.image_metrics(u8(10, 32, 3), u8(10, 32, 3))                                 # h = 10
    with pytest.raises(ValueError, match='smaller than'):
        M.image_metrics(u8(2, 32, 10, 3), u8(2, 32, 10, 3))
    with pytest.raises(ValueError, match='channels'):
        M.image_metrics(u8(16, 16, 5), u8(16, 16, 5))                                 # C = 5
    with pytest.raises(ValueError, match='differ in shape'):
        M.image_metrics(u8(16, 16, 3), u8(16, 17, 3))
    with pytest.raises(ValueError):
        M.image_metrics(u8(16, 16), u8(16, 16))
    with pytest.raises(TypeError):
        M.image_metrics(torch.zeros(16, 16, 3, dtype=torch.float64), torch.zeros(16, 16, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        M.image_metrics(np.zeros((16, 16, 3), np.uint8), np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(ValueError, match='GPU'):
        M.image_metrics(u8(16, 16, 3), u8(16, 16, 3))                                 # a valid pair, but on the host
    for f in (M.compute_psnr, M.structural_similarity):
        with pytest.raises(ValueError):
            f(u8(10, 10, 3), u8(10, 10, 3))
    with pytest.raises(ValueError, match='GPU'):
        M.color_map_backward(torch.zeros(4, 4, 3))                                    # no host path for float images
    with pytest.raises(TypeError):
        M.color_map_backward(torch.zeros(4, 4, 3, dtype=torch.float64))
    # a tensor that is not contiguous is judged by its logical shape (image_metrics copies it into a contiguous one before the kernel sees it:
    # tests/test_metrics_gpu.py::test_non_contiguous_inputs_are_read_by_their_logical_layout)
    nc = u8(3, 20, 16).permute(1, 2, 0)
    assert not nc.is_contiguous()
    with pytest.raises(ValueError, match='GPU'):
        M.image_metrics(nc, nc)
    with pytest.raises(ValueError, match='smaller than'):
        M.image_metrics(u8(3, 20, 10).permute(1, 2, 0), u8(3, 20, 10).permute(1, 2, 0))
    t = u8(4, 4, 3)
    assert M.color_map_backward(t) is t
    with pytest.raises(ValueError):
        M.ShapeRenderMetrics({'vis_format': 'bmp'})


def test_eval_images_cli_argument_handling(tmp_path):
    import subprocess
    import sys
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_images.py'), *a], capture_output=True, text=True, cwd=ROOT)
    assert run('--help').returncode == 0
    p = run('--pr', str(tmp_path / 'missing.png'), '--gt', str(tmp_path / 'missing.png'))
    assert p.returncode != 0 and 'does not exist' in p.stderr
