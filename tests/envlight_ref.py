"""Restatements for the environment-light tests (test infrastructure; no GPU): the lat-long direction grid in float64, the truth of a panorama
(the Stage-II / Stage-I oracles in float64 on that grid), the case recipes of tests/golden/env_light.npz (scripts/gen_golden_envlight.py), the
error and tolerance rule, and Radiance RGBE in numpy."""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'env_light.npz')
TOL = 1e-4                  # the project's output tolerance
FLOOR_FACTOR = 3.0          # tests/helpers.py floor_factor
SRGB_KNEE = 0.0031308

# ---- the fixture's cases: name -> recipe ------------------------------------------------------------------------------------------------------
# every model is: seed + shader_cfg of mat_bell.npz (with outer_light_version / is_real / light_exp_max of the case) -> MCShadingNetwork ->
# perturb_state(net, None) -> the recipe's edits of the state
RECIPES = {
    'plain': {},
    'clamp': {'light_exp_max': -0.7},
    'toe': {'bias_shift': -5.08},
    'gain': {'weight_g_scale': 2.0},
}
VERSIONS = ('direction', 'sphere_direction')
SMALL_SIZES = ((1, 1), (1, 5), (3, 1), (2, 2))


def case_list():
    """[(name, dict(version, is_real, recipe, h, w))] in the fixture's order"""
    cases = []
    for rec in RECIPES:
        for ver in VERSIONS:
            for real in (False, True):
                cases.append((f'{rec}_{ver}_{"real" if real else "syn"}', dict(version=ver, is_real=real, recipe=rec, h=16, w=32)))
    cases.append(('zaxis_direction_syn', dict(version='direction', is_real=False, recipe='plain', h=17, w=33)))
    for h, w in SMALL_SIZES:
        cases.append((f'size_{h}x{w}_direction_real', dict(version='direction', is_real=True, recipe='plain', h=h, w=w)))
    return cases


def case_shader_cfg(base_cfg, case):
    cfg = dict(base_cfg, outer_light_version=case['version'], is_real=bool(case['is_real']))
    rec = RECIPES[case['recipe']]
    if 'light_exp_max' in rec:
        cfg['light_exp_max'] = rec['light_exp_max']
    return cfg


def apply_recipe(holder, recipe):
    """the recipe's edits, on any module with a `shader_network.outer_light` Sequential of weight-normed Linears at 0, 2, 4, 6 (the
    reference's and the product's alike)"""
    rec = RECIPES[recipe]
    ol = holder.shader_network.outer_light
    with torch.no_grad():
        if 'bias_shift' in rec:
            ol[6].bias.add_(rec['bias_shift'])
        if 'weight_g_scale' in rec:
            for i in (0, 2, 4, 6):
                ol[i].weight_g.mul_(rec['weight_g_scale'])
    return holder


def load_fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z['meta']))


# ---- the grid and the truth -------------------------------------------------------------------------------------------------------------------
def latlong_grid(h, w, is_real):
    """float64 [h, w, 3]: network/field.py:1021-1034 with float64 linspaces"""
    az = np.linspace(1.0, 0.0, w) * np.pi * 2 - np.pi / 2 if w > 1 else np.array([1.0 * np.pi * 2 - np.pi / 2])
    el = np.linspace(1.0, -1.0, h) * np.pi / 2 if h > 1 else np.array([np.pi / 2])
    el, az = np.meshgrid(el, az, indexing='ij')
    if is_real:
        d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    else:
        d = np.stack([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)], -1)
    return d


def effective(state_dict, dtype):
    from oracle import nero_oracle as O
    return O.effective_params({k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in state_dict.items()})


def truth_stage2(state_dict, shader_cfg, dirs, gamma, dtype=torch.float64):
    """oracle.nero_oracle_mat.outer_lights at points 0 and the given directions [..., 3] (numpy float64) -> numpy [..., 3] in `dtype`"""
    from oracle import nero_oracle as O
    from oracle import nero_oracle_mat as OM
    cfg = {**OM.DEFAULT_SHADER_CFG, **shader_cfg}
    d = torch.from_numpy(np.ascontiguousarray(dirs)).to(dtype).reshape(-1, 3)
    with torch.no_grad():
        lin = OM.outer_lights(effective(state_dict, dtype), cfg, torch.zeros_like(d), d)
        out = O.linear_to_srgb(lin) if gamma else lin
    return out.reshape(dirs.shape).numpy()


def truth_stage1(state_dict, sphere, exp_max, dirs, roughness, gamma, dtype=torch.float64, bias_shift=0.0):
    """AppShadingNetwork.outer_light on IDE(d, roughness) (twice with sphere_direction), oracle.nero_oracle ide + predictor -> numpy [..., 3].
    Also returns the raw (pre-activation) head, for the clamp share."""
    from oracle import nero_oracle as O
    P = effective(state_dict, dtype)
    d = torch.from_numpy(np.ascontiguousarray(dirs)).to(dtype).reshape(-1, 3)
    with torch.no_grad():
        enc = O.ide(d, float(roughness))
        x = torch.cat([enc, enc], -1) if sphere else enc
        raw = O.predictor(P, 'color_network.outer_light', x, lambda t: t) + bias_shift
        lin = torch.exp(torch.clamp(raw, max=exp_max))
        out = O.linear_to_srgb(lin) if gamma else lin
    return out.reshape(dirs.shape).numpy(), raw.reshape(dirs.shape).numpy()


def rel_error(p, t, skip=None):
    """the largest pointwise |p - t| / t; `skip`: a (row, column) left out (the reference's NaN pixel)"""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    e = np.abs(p - t) / t
    if skip is not None:
        e = e.copy()
        e[skip[0], skip[1]] = 0.0
    return float(e.max())


def tolerance(floor):
    return max(TOL, FLOOR_FACTOR * floor)


# ---- Radiance RGBE in numpy -------------------------------------------------------------------------------------------------------------------
def rgbe_encode(x):
    """float32 [..., 3] -> uint8 [..., 4] by the definition of include/nero_hip.h (nero_env_rgbe): v = the largest channel (negative channels
    count as 0) = m 2^e, m in [0.5, 1): bytes trunc(c 2^(8 - e)), e + 128; (0, 0, 0, 0) when v < 1e-32; v >= 2^127 saturates at e = 127, bytes
    capped at 255"""
    x = np.asarray(x, np.float32)
    ch = np.maximum(x, np.float32(0))
    v = ch.max(-1)
    out = np.zeros(x.shape[:-1] + (4,), np.uint8)
    for idx in np.ndindex(v.shape):
        if not v[idx] >= np.float32(1e-32):
            continue
        _, e = np.frexp(v[idx])
        e = min(int(e), 127)
        scale = np.float32(2.0) ** np.float32(8 - e)
        for c in range(3):
            out[idx + (c,)] = min(int(np.float32(ch[idx + (c,)] * scale)), 255)
        out[idx + (3,)] = e + 128
    return out


def rgbe_decode(b):
    b = np.asarray(b)
    return np.ldexp(b[..., :3].astype(np.float64), b[..., 3:4].astype(np.int64) - 136)


def rle_scanline(line):
    """[w, 4] bytes -> one new-style run-length scanline: runs of >= 3 equal bytes as (128 + n, value), the rest as literal blocks of <= 128"""
    w = line.shape[0]
    out = bytearray([2, 2, w >> 8, w & 255])
    for c in range(4):
        col = [int(v) for v in line[:, c]]
        x = 0
        while x < w:
            run = 1
            while x + run < w and run < 127 and col[x + run] == col[x]:
                run += 1
            if run >= 3:
                out += bytes([128 + run, col[x]])
                x += run
                continue
            lit = []
            while x < w and len(lit) < 128:
                run = 1
                while x + run < w and run < 3 and col[x + run] == col[x]:
                    run += 1
                if run >= 3:
                    break
                lit.append(col[x])
                x += 1
            out += bytes([len(lit)]) + bytes(lit)
    return bytes(out)
