"""Config-surface fixtures of tests/test_config_surface.py, taken from the UNMODIFIED reference:

  python oracle/gen_golden_configs.py REFERENCE_ROOT

  tests/golden/configs/shape/*/*.yaml, material/*/*.yaml, custom/*.yaml   the reference's training YAMLs, byte for byte (settings only)
  tests/golden/ref_std_act.json      SingleVarianceNetwork(v, act)(x) of the reference (network/field.py:184-198), evaluated under
                                     oracle/ref_shim.py, for every activation and initial variance the test checks

TEST INFRASTRUCTURE ONLY: the committed fixtures are what the tests read.
"""
import glob
import json
import os
import shutil
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden')
PATTERNS = ('shape/*/*.yaml', 'material/*/*.yaml', 'custom/*shape*.yaml', 'custom/*material*.yaml')
STD_ACTS, VARIANCES = ('exp', 'linear', 'square'), (0.3, 0.07, 2.0)


def copy_configs(ref):
    src = os.path.join(ref, 'configs')
    for pat in PATTERNS:
        for path in sorted(glob.glob(os.path.join(src, pat))):
            dst = os.path.join(OUT, 'configs', os.path.relpath(path, src))
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(path, dst)


def std_act_values():
    """(oracle/ref_shim.py reads the reference root from $NERO_REFERENCE_ROOT)"""
    import torch
    from oracle import ref_shim
    _, field = ref_shim.load_reference(force_cpu=True)
    return {act: {repr(v): float(field.SingleVarianceNetwork(v, act)(torch.zeros(1, 3))[0, 0]) for v in VARIANCES} for act in STD_ACTS}


if __name__ == '__main__':
    ref = os.path.abspath(sys.argv[1])
    os.environ['NERO_REFERENCE_ROOT'] = ref
    sys.path.insert(0, REPO)
    copy_configs(ref)
    vals = std_act_values()
    with open(os.path.join(OUT, 'ref_std_act.json'), 'w') as f:
        json.dump(vals, f, indent=1)
    print('configs + ref_std_act.json written under', OUT)
