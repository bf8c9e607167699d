"""Dump tests/golden/relight_poses.npz: the output of the reference's generate_relghting_poses (blender_backend/blender_utils.py) for two
argument sets -- what nero_amd.relight.relighting_poses and tests/relight_ref.relighting_poses are compared with.

    python scripts/gen_golden_relight.py --reference /path/to/NeRO

Needs a checkout of the reference; `bpy` (Blender's Python module, which blender_utils imports at the top and the pose function never
touches) is replaced by an empty stand-in.  The tests read only the fixture."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ((8, 0.0, 30.0, 3.0), (5, 120.0, -15.0, 2.5))            # (num, azimuth, elevation, dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'relight_poses.npz'))
    a = ap.parse_args()
    sys.modules.setdefault('bpy', types.ModuleType('bpy'))
    sys.path.insert(0, os.path.join(a.reference, 'blender_backend'))
    import blender_utils
    out = {'args': np.asarray(ARGS, np.float64)}
    for i, (num, az, el, dist) in enumerate(ARGS):
        out[f'poses{i}'] = np.asarray(blender_utils.generate_relghting_poses(num, az, el, dist), np.float64)
    np.savez(a.out, **out)
    print(a.out, {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
