#!/usr/bin/env python
"""(no GPU; needs the reference tree) the fixture tests/golden/env_light.npz: what the UNMODIFIED reference's MCShadingNetwork.env_light
(network/field.py:1020-1047) returns on the CPU, through oracle/ref_shim.py, for the cases of tests/envlight_ref.py.

Every case is built in three steps, so that the tests rebuild the same weights with tests.helpers.build_material_case and none are stored:
mat_bell.npz's seed and shader_cfg (with the case's outer_light_version / is_real / light_exp_max) -> MCShadingNetwork -> perturb_state(net,
None) -> the case's recipe (tests/envlight_ref.py::apply_recipe).  Stored per case: lin/<name>, gam/<name> = env_light(h, w, gamma=False / True)
as float32 [h, w, 3], ck/<name>/<tensor> = the state checksums of the outer_light tensors; meta = the cfgs, recipes, sizes, the NaN pixel of
the 17 x 33 synthetic case and the measured conditions.  The conditions the tests re-assert are asserted here first.
Usage: python scripts/gen_golden_envlight.py [--out tests/golden/env_light.npz]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'env_light.npz'))
    args = ap.parse_args()
    out_path = os.path.abspath(args.out)
    from oracle import ref_shim
    from oracle.golden_util import perturb_state, state_checksums
    from tests import envlight_ref as R
    from tests.helpers import load_golden
    _, base = load_golden('mat_bell')
    _, field = ref_shim.load_reference()
    import torch.nn as nn

    class Holder(nn.Module):
        pass
    rec, meta = {}, {'seed': base['seed'], 'base': 'mat_bell', 'cases': {}}
    for name, case in R.case_list():
        cfg = R.case_shader_cfg(base['shader_cfg'], case)
        torch.manual_seed(base['seed'])
        net = Holder()
        net.shader_network = field.MCShadingNetwork(cfg, None)
        perturb_state(net, None)
        R.apply_recipe(net, case['recipe'])
        h, w = case['h'], case['w']
        with torch.no_grad():
            lin = net.shader_network.env_light(h, w, gamma=False).numpy().astype(np.float32)
            gam = net.shader_network.env_light(h, w, gamma=True).numpy().astype(np.float32)
        assert lin.shape == (h, w, 3) and gam.shape == (h, w, 3)
        nan = np.argwhere(np.isnan(lin).any(-1))
        info = dict(case, shader_cfg=cfg, nan_pixel=None)
        if name.startswith('zaxis'):
            assert len(nan) == 1 and tuple(nan[0]) == (8, 24), nan
            assert np.array_equal(np.isnan(gam).any(-1), np.isnan(lin).any(-1))
            info['nan_pixel'] = [int(nan[0][0]), int(nan[0][1])]
        else:
            assert len(nan) == 0 and not np.isnan(gam).any(), (name, nan)
        fin = lin[~np.isnan(lin).any(-1)]
        info['max_over_min'] = float(fin.max() / fin.min())
        emax = {**field.MCShadingNetwork.default_cfg, **cfg}['light_exp_max']
        info['clamped_share'] = float((fin >= np.float32(np.exp(emax)) * (1 - 1e-6)).mean())
        info['below_knee_share'] = float((fin <= R.SRGB_KNEE).mean())
        # (a clamp case has the weights of its plain case and a ceiling of exp(-0.7) on top: its own max / min is cut by the ceiling, so the
        #  variation of its network is what the plain case of the same name shows; the maps of a few pixels are there for their sizes)
        if case['recipe'] != 'clamp' and h * w >= 512:
            assert info['max_over_min'] >= 1.03, (name, info['max_over_min'])
        if case['recipe'] == 'gain':
            assert info['max_over_min'] >= 1.5, (name, info['max_over_min'])
        if case['recipe'] == 'clamp':
            assert 0.1 <= info['clamped_share'] <= 0.9, (name, info['clamped_share'])
        if case['recipe'] == 'toe':
            assert 0.1 <= info['below_knee_share'] <= 0.9, (name, info['below_knee_share'])
        rec['lin/' + name], rec['gam/' + name] = lin, gam
        sd = {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith('shader_network.outer_light.')}
        for k, v in state_checksums(sd).items():
            rec[f'ck/{name}/{k}'] = v
        meta['cases'][name] = info
        print(f'{name}: {h} x {w}, range {fin.min():.4g} .. {fin.max():.4g} (max/min {info["max_over_min"]:.3f}), clamped '
              f'{info["clamped_share"]:.2f}, below the sRGB knee {info["below_knee_share"]:.2f}, NaN pixel {info["nan_pixel"]}')
    rec['meta'] = json.dumps(meta)
    np.savez_compressed(out_path, **rec)
    print(f'wrote {out_path}: {os.path.getsize(out_path)} bytes')


if __name__ == '__main__':
    main()
