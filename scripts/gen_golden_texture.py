#!/usr/bin/env python
"""(no GPU; needs scipy and scikit-learn) the fixture tests/golden/texture_regions.npz: what the reference's own gutter formulation
(extract_materials_texture_map.py:136-149) gives on the seeded masks of tests/texture_ref.py, so that the tests need neither package.

Per mask m (index into texture_ref.GUTTER_MASKS) and pad p (texture_ref.GUTTER_PADS):
  mask_m                the mask, bytes [h, w]
  region_m_p            scipy's regions, called exactly as the reference calls them: binary_dilation(mask, iterations=p) with the mask taken
                        out = 3, the mask minus binary_erosion(mask, iterations=3) = 2, the rest of the mask = 1
  d2_m_p, src_m_p       for every fill texel in row-major order: sklearn's kd-tree nearest distance, squared and rounded to the integer it is,
                        and the row-major index of the search texel it chose (ties: whichever the tree met first)
Usage: python scripts/gen_golden_texture.py [--out tests/golden/texture_regions.npz]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'texture_regions.npz'))
    args = ap.parse_args()
    from scipy.ndimage import binary_dilation, binary_erosion
    from sklearn.neighbors import NearestNeighbors
    from tests import texture_ref as R
    rec = {}
    for m, (h, w, seed) in enumerate(R.GUTTER_MASKS):
        mask = R.gutter_mask(h, w, seed)
        rec[f'mask_{m}'] = mask.astype(np.uint8)
        for pad in R.GUTTER_PADS:
            inpaint = binary_dilation(mask, iterations=pad)
            inpaint[mask] = 0
            search = mask.copy()
            search[binary_erosion(search, iterations=3)] = 0
            region = mask.astype(np.uint8)
            region[search] = 2
            region[inpaint] = 3
            sc = np.stack(np.nonzero(search), -1)
            ic = np.stack(np.nonzero(inpaint), -1)
            dist, ind = NearestNeighbors(n_neighbors=1, algorithm='kd_tree').fit(sc).kneighbors(ic)
            d2 = np.rint(dist[:, 0] ** 2).astype(np.int32)
            assert np.abs(dist[:, 0] ** 2 - d2).max() < 1e-6
            chosen = sc[ind[:, 0]]
            rec[f'region_{m}_{pad}'] = region
            rec[f'd2_{m}_{pad}'] = d2
            rec[f'src_{m}_{pad}'] = (chosen[:, 0] * w + chosen[:, 1]).astype(np.int32)
            print(f'mask {m} ({h} x {w}) pad {pad}: {int(mask.sum())} covered, {len(sc)} search, {len(ic)} fill texels, largest nearest distance '
                  f'{float(dist.max()):.1f}')
    np.savez_compressed(args.out, **rec)
    print(f'wrote {args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
