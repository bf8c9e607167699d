"""Validation on the device (libnero_hip.so, nero_img_*): PSNR, SSIM and the picture panel of a validation view.

The reference does this in network/metrics.py and train/train_valid.py: every float image of a view is copied to the host, quantised there
(color_map_backward), scored with a float32 PSNR and skimage's structural_similarity, and written as a JPEG panel with skimage's imsave.
Here the images that NeROShapeRenderer.test_step / NeROMaterialRenderer.test_step return stay on the device:
  * color_map_backward: float32 -> uint8 (nero_img_quantize);
  * image_metrics / compute_psnr / structural_similarity: the exact PSNR and the SSIM of 8-bit images (nero_img_metrics), no host
    synchronisation until the caller reads the numbers;
  * concat_images_list / draw_materials: the panel layout (utils/draw_utils.py:163-183, network/metrics.py:19-37) as tensor glue, on the
    device or on the host;
  * ShapeRenderMetrics / MaterialRenderMetrics, name2metrics, name2key_metrics: the call contract of network/metrics.py:39-115;
  * ValidationEvaluator: the call contract of train/train_valid.py:18-52.
SSIM follows this project's statement of skimage's algorithm (include/nero_hip.h); skimage is not a dependency.  PSNR is the exact value in
float64: the reference's float32 mean is up to 2e-3 dB off it at 800 x 800."""
import os

import numpy as np
import torch

from . import _lib as L

_lib = L.lib

WIN = 11                    # the SSIM window the reference passes to skimage
MAX_SIZE, MAX_BATCH, MAX_CHANNELS = 16384, 65535, 4


# ---- kernels --------------------------------------------------------------------------------------------------------------------------------
def color_map_backward(x):
    """float32 device tensor in [0, 1] -> uint8 tensor of the same shape: uint8(clip(x * 255, 0, 255)), truncated (nero_img_quantize;
    utils/base_utils.py:453-456).  NaN -> 0 by this project's definition (numpy leaves it undefined), +inf -> 255, -inf -> 0.  A uint8 tensor
    is returned as it is, on any device.  Anything else raises before a launch: there is no host path for float images."""
    if not torch.is_tensor(x):
        raise TypeError(f'color_map_backward: a torch tensor is expected, got {type(x).__name__}')
    if x.dtype == torch.uint8:
        return x
    if x.dtype != torch.float32:
        raise TypeError(f'color_map_backward: float32 or uint8 expected, got {x.dtype}')
    if not x.is_cuda:
        raise ValueError('color_map_backward: float images are quantised on the GPU; got a host tensor')
    x = x.detach().contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        L.check(_lib.nero_img_quantize(L.ptr(x), x.numel(), L.ptr(out), L.stream_ptr()))
    return out


def _check_pair(gt, pr):
    """dtype, shape and size -- then the device -- of an image pair, before anything is launched; -> (B, h, w, C)"""
    for name, t in (('gt', gt), ('pr', pr)):
        if not torch.is_tensor(t):
            raise TypeError(f'image_metrics: {name} must be a torch tensor, got {type(t).__name__}')
        if t.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f'image_metrics: {name} must be float32 (in [0, 1]) or uint8, got {t.dtype}')
    if gt.shape != pr.shape:
        raise ValueError(f'image_metrics: the images differ in shape: {tuple(gt.shape)} and {tuple(pr.shape)}')
    if gt.dim() not in (3, 4):
        raise ValueError(f'image_metrics: [h, w, C] or [B, h, w, C] expected, got {tuple(gt.shape)}')
    B = 1 if gt.dim() == 3 else gt.shape[0]
    h, w, Cn = gt.shape[-3:]
    if not 1 <= Cn <= MAX_CHANNELS:
        raise ValueError(f'image_metrics: 1 to {MAX_CHANNELS} channels expected (last axis), got {Cn}')
    if min(h, w) < WIN:
        raise ValueError(f'image_metrics: a {h} x {w} image is smaller than the {WIN} x {WIN} SSIM window')
    if max(h, w) > MAX_SIZE or not 1 <= B <= MAX_BATCH:
        raise ValueError(f'image_metrics: at most {MAX_SIZE} pixels on a side and 1 to {MAX_BATCH} images, got {tuple(gt.shape)}')
    if not (gt.is_cuda and pr.is_cuda and gt.device == pr.device):
        raise ValueError(f'image_metrics: both images must be on the same GPU, got {gt.device} and {pr.device}')
    return B, h, w, Cn


def image_metrics(gt, pr, details=False):
    """gt, pr: [h, w, C] or [B, h, w, C] device tensors, float32 in [0, 1] (quantised first, color_map_backward) or uint8, C in 1..4, h and w
    in 11..16384 -> float64 device tensor [B, 2] = (psnr, ssim) per image (nero_img_metrics).  Nothing is copied to the host and nothing
    synchronises.  psnr = 10 log10(65025 / mse) from the exact integer sum of squared differences, +inf for identical images; ssim as
    skimage.metrics.structural_similarity(gt, pr, win_size=11, channel_axis=2, data_range=255).  details: -> (out, sse int64 [B], ssim_c
    float64 [B, C]).  A wrong dtype, shape or device raises TypeError / ValueError before any launch; tensors that are not contiguous are
    copied into contiguous ones."""
    B, h, w, Cn = _check_pair(gt, pr)
    dev = gt.device
    with torch.cuda.device(dev):
        g, p = color_map_backward(gt).contiguous(), color_map_backward(pr).contiguous()
        ws = torch.empty(max(int(_lib.nero_img_metrics_workspace_bytes(B, h, w, Cn)), 256), dtype=torch.uint8, device=dev)
        out = torch.empty((B, 2), dtype=torch.float64, device=dev)
        sse = torch.empty(B, dtype=torch.int64, device=dev) if details else None          # (below 2^47: the same bits as the uint64)
        ssim_c = torch.empty((B, Cn), dtype=torch.float64, device=dev) if details else None
        L.check(_lib.nero_img_metrics(L.ptr(g), L.ptr(p), B, h, w, Cn, L.ptr(ws), L.ptr(sse), L.ptr(ssim_c), L.ptr(out), L.stream_ptr()))
    return (out, sse, ssim_c) if details else out


def _column(gt, pr, col):
    v = image_metrics(gt, pr)[:, col].cpu().numpy()
    return float(v[0]) if gt.dim() == 3 else v


def compute_psnr(gt, pr):
    """-> the PSNR in dB as a Python float (a float64 array [B] for a batch); network/metrics.py:11-17 without its float32 rounding"""
    return _column(gt, pr, 0)


def structural_similarity(gt, pr):
    """-> the SSIM as a Python float (a float64 array [B] for a batch), as the reference calls skimage's function"""
    return _column(gt, pr, 1)


# ---- panels ---------------------------------------------------------------------------------------------------------------------------------
def _pad_to(img, h, w):
    if img.shape[0] == h and img.shape[1] == w:
        return img
    out = torch.zeros((h, w) + tuple(img.shape[2:]), dtype=img.dtype, device=img.device)
    out[:img.shape[0], :img.shape[1]] = img
    return out


def concat_images_list(*imgs, vert=False):
    """uint8 tensors [h, w, C] side by side (vert: one below the other), the shorter (narrower) ones zero-padded at the bottom (right):
    utils/draw_utils.py:163-183.  Works on device and on host tensors."""
    if not imgs:
        raise ValueError('concat_images_list: no image given')
    for im in imgs:
        if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3:
            raise TypeError('concat_images_list: uint8 tensors [h, w, C] expected')
    if len(imgs) == 1:
        return imgs[0]
    if vert:
        w = max(im.shape[1] for im in imgs)
        return torch.cat([_pad_to(im, im.shape[0], w) for im in imgs], 0)
    h = max(im.shape[0] for im in imgs)
    return torch.cat([_pad_to(im, h, im.shape[1]) for im in imgs], 1)


def process_key_img(x, h, w):
    """one output of test_step -> uint8 [h, w, 3]: quantised, a single channel repeated to three (network/metrics.py:19-23)"""
    img = color_map_backward(x.detach()).reshape(h, w, -1)
    return img.repeat(1, 1, 3) if img.shape[-1] == 1 else img


def get_key_images(data_pr, keys, h, w):
    return [process_key_img(data_pr[k], h, w) for k in keys if k in data_pr]


MATERIAL_KEYS = ['diffuse_albedo', 'diffuse_light', 'diffuse_color', 'specular_albedo', 'specular_light', 'specular_color', 'specular_ref',
                 'metallic', 'roughness', 'occ_prob', 'indirect_light']


def draw_materials(data_pr, h, w):
    """the shader intermediates of a Stage-I validation view as up to three panel rows (network/metrics.py:31-37): the images of the keys that
    are present, in the order of MATERIAL_KEYS, cut 3 / 4 / the rest.  Absent keys are skipped and an empty row is dropped (the reference
    would fail on one)."""
    imgs = get_key_images(data_pr, MATERIAL_KEYS, h, w)
    return [concat_images_list(*row) for row in (imgs[0:3], imgs[3:7], imgs[7:]) if row]


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


class _RenderMetrics:
    """what the two metric classes share: the configuration, the scores and the panel file"""
    default_cfg = {'vis_dir': 'data/train_vis', 'vis_format': None, 'write_vis': True}

    def __init__(self, cfg=None):
        self.cfg = {**self.default_cfg, **(cfg or {})}
        fmt = self.cfg['vis_format']
        if fmt is None:
            fmt = 'jpg' if _pil() is not None else 'png'
        if fmt not in ('jpg', 'png'):
            raise ValueError(f"vis_format must be 'jpg' or 'png', got {fmt!r}")
        if fmt == 'jpg' and _pil() is None:
            raise ImportError("vis_format 'jpg' needs PIL; use 'png'")
        self.vis_format = fmt

    def _finish(self, gt, pr, rows, step, kwargs):
        scores = image_metrics(gt, pr)                                   # queued; read below
        panel = concat_images_list(*rows, vert=True) if self.cfg['write_vis'] else None
        scores = scores.cpu().numpy()                                    # the one copy of the numbers
        if panel is not None:
            out_dir = os.path.join(self.cfg['vis_dir'], str(kwargs['model_name']))
            os.makedirs(out_dir, exist_ok=True)
            path = os.path.join(out_dir, f"{step}-index-{kwargs['data_index']}.{self.vis_format}")
            img = np.ascontiguousarray(panel.cpu().numpy())
            if self.vis_format == 'jpg':
                _pil().fromarray(img).save(path, format='JPEG')
            else:
                from .texture import write_png
                write_png(path, img)
        return {'psnr': np.asarray([scores[0, 0]]), 'ssim': np.asarray([scores[0, 1]])}


class ShapeRenderMetrics(_RenderMetrics):
    """network/metrics.py:39-72 on the outputs of NeROShapeRenderer.test_step: (data_pr, data_gt, step, data_index=, model_name=) ->
    {'psnr': float64 [1], 'ssim': float64 [1]}, and the panel {vis_dir}/{model_name}/{step}-index-{data_index}.{ext}: gt_rgb | ray_rgb | normal
    | human_light over the rows of draw_materials.  cfg: vis_dir ('data/train_vis'), vis_format ('jpg' through PIL when it imports, else 'png'),
    write_vis (True)."""

    def __call__(self, data_pr, data_gt, step, **kwargs):
        gt, pr = color_map_backward(data_pr['gt_rgb'].detach()), color_map_backward(data_pr['ray_rgb'].detach())
        if pr.dim() != 3 or gt.shape != pr.shape:
            raise ValueError(f'ShapeRenderMetrics: gt_rgb and ray_rgb must both be [h, w, 3], got {tuple(gt.shape)} and {tuple(pr.shape)}')
        rows = []
        if self.cfg['write_vis']:
            h, w, _ = pr.shape
            rows = [concat_images_list(gt, pr, *get_key_images(data_pr, ['normal', 'human_light'], h, w))] + draw_materials(data_pr, h, w)
        return self._finish(gt, pr, rows, step, kwargs)


class MaterialRenderMetrics(_RenderMetrics):
    """network/metrics.py:74-102 on the outputs of NeROMaterialRenderer.test_step: rgb_gt | rgb_pr | albedo | metallic | roughness over
    specular_light | specular_color | diffuse_light | diffuse_color (the present ones, cut after the fifth image)."""
    additional_keys = ['albedo', 'metallic', 'roughness', 'specular_light', 'specular_color', 'diffuse_light', 'diffuse_color']

    def __call__(self, data_pr, data_gt, step, *args, **kwargs):
        gt, pr = color_map_backward(data_pr['rgb_gt'].detach()), color_map_backward(data_pr['rgb_pr'].detach())
        if pr.dim() != 3 or gt.shape != pr.shape:
            raise ValueError(f'MaterialRenderMetrics: rgb_gt and rgb_pr must both be [h, w, 3], got {tuple(gt.shape)} and {tuple(pr.shape)}')
        rows = []
        if self.cfg['write_vis']:
            h, w, _ = pr.shape
            imgs = [gt, pr] + get_key_images(data_pr, self.additional_keys, h, w)
            rows = [concat_images_list(*row) for row in (imgs[:5], imgs[5:]) if row]
        return self._finish(gt, pr, rows, step, kwargs)


name2metrics = {
    'shape_render': ShapeRenderMetrics,
    'mat_render': MaterialRenderMetrics,
}


def psnr(results):
    return np.mean(results['psnr'])


name2key_metrics = {
    'psnr': psnr,
}


# ---- the validation loop --------------------------------------------------------------------------------------------------------------------
class ValidationEvaluator:
    """train/train_valid.py:11-52: evaluator(model, losses, eval_dataset, step, model_name, val_set_name=None) -> (eval_results,
    key_metric_value).  eval_dataset: an iterable of {'index': i} dicts (what the reference's DummyDataset yields); each is passed to the model
    with 'eval' and 'step' set, under no_grad; every metric of `losses` is applied to the outputs; the per-view results are concatenated and
    the key metric (cfg['key_metric_name']) is added under its name."""
    default_cfg = {}

    def __init__(self, cfg):
        self.cfg = {**self.default_cfg, **cfg}
        self.key_metric_name = cfg['key_metric_name']
        self.key_metric = name2key_metrics[self.key_metric_name]

    def __call__(self, model, losses, eval_dataset, step, model_name, val_set_name=None):
        if val_set_name is not None:
            model_name = f'{model_name}-{val_set_name}'
        model.eval()
        eval_results = {}
        for data_i, data in enumerate(eval_dataset):
            data = dict(data)
            data['eval'] = True
            data['step'] = step
            with torch.no_grad():
                outputs = model(data)
            for loss in losses:
                for k, v in loss(outputs, data, step, data_index=data_i, model_name=model_name).items():
                    if torch.is_tensor(v):
                        v = v.detach().cpu().numpy()
                    eval_results.setdefault(k, []).append(v)
        for k, v in eval_results.items():
            eval_results[k] = np.concatenate(v, axis=0)
        key_metric_val = self.key_metric(eval_results)
        eval_results[self.key_metric_name] = key_metric_val
        return eval_results, key_metric_val
