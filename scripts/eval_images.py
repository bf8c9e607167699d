"""PSNR and SSIM of rendered images against ground truth on the GPU (nero_amd/metrics.py), as the reference's validation scores them
(network/metrics.py: compute_psnr, structural_similarity(win_size=11, channel_axis=2, data_range=255)):

    python scripts/eval_images.py --pr A.png --gt B.png
    python scripts/eval_images.py --pr DIR_A --gt DIR_B [--json scores.json]
        two PNG files, or two directories whose *.png files are paired by name (names present in only one of them are reported and skipped).

Prints `<name> <psnr:.4f> <ssim:.6f>` per pair and the means (over the pairs with a finite PSNR for the PSNR).  8-bit grey / RGB / RGBA PNGs, read
without PIL (nero_amd.texture.read_png)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pairs_of(pr, gt):
    if os.path.isdir(pr) != os.path.isdir(gt):
        sys.exit('eval_images: --pr and --gt must be two files or two directories')
    if not os.path.isdir(pr):
        return [(os.path.basename(pr), pr, gt)]
    names = lambda d: {f for f in os.listdir(d) if f.lower().endswith('.png')}
    a, b = names(pr), names(gt)
    for f in sorted(a ^ b):
        print(f'eval_images: {f} is in only one of the directories, skipped', file=sys.stderr)
    if not a & b:
        sys.exit('eval_images: the directories share no *.png file name')
    return [(f, os.path.join(pr, f), os.path.join(gt, f)) for f in sorted(a & b)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pr', type=str, required=True, help='rendered image (PNG) or a directory of them')
    ap.add_argument('--gt', type=str, required=True, help='ground-truth image (PNG) or a directory of them')
    ap.add_argument('--json', type=str, default=None, help='also write the scores to this file')
    a = ap.parse_args(argv)
    for path in (a.pr, a.gt):
        if not os.path.exists(path):
            sys.exit(f'eval_images: {path} does not exist')
    pairs = pairs_of(a.pr, a.gt)
    import torch
    from nero_amd import metrics as M
    from nero_amd.texture import read_png
    if not torch.cuda.is_available():
        sys.exit('eval_images: the metrics run on a GPU; none is visible')
    rows = []
    for name, p_pr, p_gt in pairs:
        imgs = []
        for p in (p_gt, p_pr):
            im = read_png(p)
            imgs.append(torch.from_numpy(np.ascontiguousarray(im if im.ndim == 3 else im[..., None])).cuda())
        if imgs[0].shape != imgs[1].shape:
            sys.exit(f'eval_images: {name}: the images differ in shape, {tuple(imgs[1].shape)} and {tuple(imgs[0].shape)}')
        psnr, ssim = M.image_metrics(imgs[0], imgs[1])[0].tolist()
        rows.append({'name': name, 'psnr': psnr, 'ssim': ssim})
        print(f'{name} {psnr:.4f} {ssim:.6f}')
    finite = [r['psnr'] for r in rows if np.isfinite(r['psnr'])]
    mean = {'psnr': float(np.mean(finite)) if finite else float('inf'), 'ssim': float(np.mean([r['ssim'] for r in rows])), 'pairs': len(rows)}
    print(f"mean {mean['psnr']:.4f} {mean['ssim']:.6f}")
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump({'pairs': rows, 'mean': mean}, fh, indent=1)
            fh.write('\n')
    return rows, mean


if __name__ == '__main__':
    main()
