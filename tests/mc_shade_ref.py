"""Plain torch restatement of the Stage-II shading and loss kernels (nero_amd/csrc/mc_shade.hip, mat_loss.hip): one function per entry
point or natural group, over the arrays the kernels take, written from the formulas with differentiable torch ops only and dtype-generic
(one source serves float64 and float32).  The raw light-MLP heads, the traced depth / hit position / face normal and the hit / miss split
(slot, miss_idx, hit_idx, n_hum) are INPUTS: no tracer and no MLP.  Backward references are torch.autograd of these forwards, so every
tie rule is torch's own.  Pieces oracle/nero_oracle.py and oracle/nero_oracle_mat.py already state are called, not restated.
tests/test_mc_shade_ref_cpu.py pins this file to the oracle; tests/test_mc_shade_kernels_gpu.py compares the kernels with it.

`wrong`: the name of one deliberately wrong variant (WRONG below) -- the CPU tier feeds each through the judge of the GPU tier and
requires that it is rejected.

Condition classes (per surface point, `cls`): 0 = regular (roughness in [0.1, 0.9], NoV >= 0.1, unit normal, |p| < 0.9), 1 = extreme
(roughness 0.04^2 or 1, NoV = 0 or a back-facing view, axis-aligned or zero normal, |p| > 0.999).  Float32 floors are taken per (output,
geometry, class, fewer than 16 directions): an extreme row never loosens the bound of a regular one.

Measured float32 floors of the committed estimator input sets (worst row over EST_CASES and the row-ownership sets, float32 CPU evaluation
against float64, the larger of the two geometry terms; tests/test_mc_shade_ref_cpu.py prints the full table):
                          forward   d_roughness  d_metallic  d_albedo  raw-head rows  d_wspec
  regular, D >= 16        3.1e-5    2.9e-4       7.2e-6      1.0e-5    6.2e-5         4.5e-5
  regular, D <  16        3.6e-5    1.2e-3       7.1e-5      3.3e-5    3.3e-5         4.9e-6
  extreme, D >= 16        1.0e-5    2.4e-3       4.1e-6      1.7e-6    2.1e-5         5.3e-4
  extreme, D <  16        1.4e-5    3.5e-3       1.0e-4      6.7e-6    1.4e-5         6.1e-6
(d_mat5 components against their term sizes, raw-head rows against the larger of the row and its term sizes.)  Points with fewer than
16 directions are a condition of their own: their one or two GGX samples sit where the Fibonacci table puts them (Ds = 1: at the
grazing end), not averaged over a hemisphere."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import nero_oracle as O
from oracle import nero_oracle_mat as M
from tests.shade_ref import EPS32, leaf, row_pad, vjp  # noqa: F401  (re-exported for the two test tiers)

DEAD_SLOT = -2 ** 31
R_MIN, R_SPAN = 0.04 ** 2, 1.0 - 0.04 ** 2
WRONG = ('diffuse_over_D', 'fresnel_exp4', 'near_ignored', 'dead_lit', 'human_weight_unclamped', 'no_pull_in', 'no_q_eps', 'no_dir_bwd',
         'no_smith_dnol', 'hinge_mean', 'reg_albedo_weight_1')
F32, F64 = torch.float32, torch.float64


# ---- per-point record, directions ------------------------------------------------------------------------------------------------------
def point_setup(pts, view, normals, mat5, rand_d, rand_s):
    """-> pt [P,32] (layout: top of mc_shade.hip), decisions.  rand_* [P] in [0,1) or None (azimuth flag -1)"""
    v, n = F.normalize(view, dim=-1), F.normalize(normals, dim=-1)
    nv = (v * n).sum(-1, keepdim=True)
    refl = nv * n * 2 - v
    xd = M.orthogonal_direction(n)
    yd = torch.linalg.cross(n, xd)
    xs = M.orthogonal_direction(refl)
    ys = torch.linalg.cross(refl, xs)
    flag = lambda r: -torch.ones_like(nv) if r is None else r.reshape(-1, 1) * (2 * math.pi)
    pt = torch.cat([v, n, refl, mat5, nv.clamp(0.0, 1.0), xd, yd, xs, ys, flag(rand_d), flag(rand_s), pts], -1)

    def ortho_dist(d):
        l0, l1 = torch.sqrt(d[:, 1] ** 2 + d[:, 0] ** 2), torch.sqrt(d[:, 2] ** 2 + d[:, 0] ** 2)
        return l0 > l1, (l0 - l1).abs()
    dec = {'ortho_n': ortho_dist(n), 'ortho_r': ortho_dist(refl), 'nov0': (nv[:, 0] >= 0, nv[:, 0].abs())}
    return pt, dec


def _az(t, off):
    az = t[None, :] * (2 * math.pi)
    return torch.where(off >= 0, torch.remainder(az + off, 2 * math.pi), az)


def diffuse_dirs(pt, tab_d):
    """tab_d [Dd,2] = (azimuth, elevation) in [0,1] -> [P,Dd,3]   (cosine-weighted)"""
    az, el = _az(tab_d[:, 0], pt[:, 27:28]), tab_d[None, :, 1]
    es, cz = torch.sqrt(el + 1e-7), torch.sqrt(1 - el + 1e-7)
    cx, cy = (es * torch.cos(az))[..., None], (es * torch.sin(az))[..., None]
    return cx * pt[:, None, 15:18] + cy * pt[:, None, 18:21] + cz[..., None] * pt[:, None, 3:6]


def specular_dirs(pt, tab_s, rough=None):
    """GGX importance sampling around the reflection; rough [P,1] or [P,Ds] overrides pt[:,10] -> [P,Ds,3]"""
    a = pt[:, 10:11] if rough is None else rough
    el = tab_s[None, :, 1]
    cost = torch.sqrt((1.0 - el + 1e-6) / (1.0 + (a * a - 1.0) * el + 1e-6) + 1e-6)
    sint = torch.sqrt(1 - cost * cost + 1e-6)
    phi = _az(tab_s[:, 0], pt[:, 28:29])
    return (torch.cos(phi) * sint)[..., None] * pt[:, None, 21:24] + (torch.sin(phi) * sint)[..., None] * pt[:, None, 24:27] \
        + cost[..., None] * pt[:, None, 6:9]


def dirs(pt, tab_d, tab_s):
    """-> dirs [P*D,3], origins [P*D,3] = p + 1e-5 w   (row = p * D + j, diffuse directions first)"""
    w = torch.cat([diffuse_dirs(pt, tab_d), specular_dirs(pt, tab_s)], 1)
    o = pt[:, None, 29:32] + w * 1e-5
    return w.reshape(-1, 3), o.reshape(-1, 3)


def dead_rays(pt, dirs_, Dd, Ds, geometry_type):
    """-> dead [P*D] bool: GGX-sampled direction with n.w < -1e-6 (Schlick-GGX only), decisions"""
    D = Dd + Ds
    nw = (pt[:, None, 3:6] * dirs_.reshape(-1, D, 3)).sum(-1)
    spec = (torch.arange(D) >= Dd)[None, :]
    dead = spec & (nw < -1e-6) & (geometry_type == 0)
    return dead.reshape(-1), {'dead_margin': ((nw < -1e-6)[:, Dd:], (nw + 1e-6).abs()[:, Dd:])}


def human_geom(poses, p, w):
    """poses [n,3,4], p, w [n,3] -> mean [n,2] (not yet masked), h [n] (0 / 1), decisions"""
    inter, dist, hits0 = O.camera_plane_intersection(p, w, poses)
    mean = inter[..., :2] * 0.3
    rad = torch.norm(mean, dim=-1)
    h = (hits0 & (rad < 1.5) & (dist > 0)).to(p.dtype)
    dz = (poses[:, :, :3] @ w[:, :, None])[:, 2, 0]
    dec = {'dz_small': (dz.abs() > 1e-4, (dz.abs() - 1e-4).abs()), 'dist_pos': (dist > 0, dist.abs()), 'radius': (rad < 1.5, (rad - 1.5).abs())}
    return mean, h, dec


def human_flags(pt, dirs_, poses, D):
    """poses [P,3,4] -> hum [P*D] bool, decisions"""
    pi = torch.arange(dirs_.shape[0]) // D
    _, h, dec = human_geom(poses[pi], pt[pi, 29:32], dirs_)
    return h != 0, dec


# ---- light-MLP inputs as functions of the direction ----------------------------------------------------------------------------------------
def miss_rows(w, p, sphere, wrong=''):
    """w, p [n,3] -> X [n,72|144] = IDE(w, 0) [| IDE(exit point of (p', w) on the unit sphere, 0)], p' = 0.999 p when |p| > 0.999"""
    X = O.ide(w, 0.0)
    if sphere:
        far = torch.norm(p, dim=-1, keepdim=True) > 0.999
        pp = p if wrong == 'no_pull_in' else torch.where(far, p * 0.999, p)
        X = torch.cat([X, O.ide(pp + w * O.sphere_exit_dist(pp, w), 0.0)], -1)
    return X


def human_rows(w, p, poses):
    """-> Xh [n,24] = IPE(0.3 h inter_xy, 0) degrees 0..5, hmask [n]"""
    mean, h, _ = human_geom(poses, p, w)
    mean = mean * h[:, None]
    return O.ipe(mean, torch.zeros_like(mean), 0, 6), h


def hit_rows(w, pos, fnrm):
    """-> X [n,128] = [PE-8(x_hit) 51 | IDE(reflect(-w about -normalize(face normal)), 0) 72 | 0 x 5]"""
    nh = F.normalize(-fnrm, dim=-1)                                          # (the kernel normalises twice, as trace() and get_inner_lights do: idempotent)
    vv = F.normalize(-w, dim=-1)
    refl = (vv * nh).sum(-1, keepdim=True) * nh * 2 - vv
    return torch.cat([O.pos_enc(pos, 8), O.ide(refl, 0.0), torch.zeros_like(w[:, :1]).expand(-1, 5)], -1)


def _pidx(idx, D):
    return torch.div(idx.long(), D, rounding_mode='floor')


def encode_miss(dirs_, idx, pt, D, sphere):
    return miss_rows(dirs_[idx.long()], pt[_pidx(idx, D), 29:32], sphere)


def human_encode(dirs_, idx, pt, D, poses):
    pi = _pidx(idx, D)
    return human_rows(dirs_[idx.long()], pt[pi, 29:32], poses[pi])


def encode_hit(dirs_, pos, fnrm, idx):
    i = idx.long()
    return hit_rows(dirs_[i], pos[i], fnrm[i])


def split(depth, dead=None, hum=None):
    """the hit / miss split as nero_mc_split_classes defines it -> slot [N] int32, miss_idx, hit_idx, n_hum: hits (depth < 10, not dead) in
    ray order; misses that reach the photographer's region first (ray order), then the other misses (ray order); dead rays in neither list"""
    N = depth.shape[0]
    dead = torch.zeros(N, dtype=torch.bool) if dead is None else dead.bool()
    hum = torch.zeros(N, dtype=torch.bool) if hum is None else hum.bool()
    hit = ~dead & (depth < 10.0)
    miss = ~dead & ~hit
    hm, pm = torch.nonzero(miss & hum)[:, 0], torch.nonzero(miss & ~hum)[:, 0]
    miss_idx, hit_idx = torch.cat([hm, pm]), torch.nonzero(hit)[:, 0]
    slot = torch.full((N,), DEAD_SLOT, dtype=torch.int64)
    slot[miss_idx] = torch.arange(miss_idx.numel())
    slot[hit_idx] = -torch.arange(hit_idx.numel()) - 1
    return slot.int(), miss_idx.int(), hit_idx.int(), int(hm.numel())


# ---- the estimator --------------------------------------------------------------------------------------------------------------------------
def lights(slot, depth, outer_raw, inner_raw, human_raw, hmask, n_hum, emax, imax, wrong=''):
    """L [N,3] = near * (miss: outer (1 - hw) + hl hw, the human light for the miss rows [0, n_hum) only; hit: inner; dead: 0), decisions"""
    dt = outer_raw.dtype
    s = slot.long()
    miss, dead = s >= 0, s == DEAD_SLOT
    hit = ~miss & ~dead
    near = torch.ones_like(depth) if wrong == 'near_ignored' else (depth > 1e-5).to(dt)
    Lm = torch.exp(torch.clamp(outer_raw[:, :3], max=emax))
    dec = {'outer_cap': (outer_raw[:, :3] <= emax, (outer_raw[:, :3] - emax).abs()), 'inner_cap': (inner_raw[:, :3] <= imax, (inner_raw[:, :3] - imax).abs()),
           'near': (depth > 1e-5, (depth - 1e-5).abs())}
    nh = 0 if human_raw is None else min(int(n_hum), Lm.shape[0])
    if nh > 0:
        h = torch.exp(torch.clamp(human_raw[:nh], max=0.0)) * hmask[:nh, None]
        hw_raw = h[:, 3:]
        hw = hw_raw if wrong == 'human_weight_unclamped' else torch.clamp(hw_raw, 0.0, 1.0)
        Lm = torch.cat([Lm[:nh] * (1 - hw) + h[:, :3] * hw, Lm[nh:]])
        dec.update(human_cap=(human_raw[:nh] <= 0, human_raw[:nh].abs()), hw_hi=(hw_raw[:, 0] <= 1, (hw_raw[:, 0] - 1).abs()),
                   hw_lo=(hw_raw[:, 0] >= 0, hw_raw[:, 0].abs()))
    Li = torch.exp(torch.clamp(inner_raw[:, :3], max=imax))
    zero = torch.zeros(1, 3, dtype=dt)
    Lm, Li = torch.cat([Lm, zero]), torch.cat([Li, zero])
    L = torch.where(miss[:, None], Lm[torch.where(miss, s, Lm.shape[0] - 1)], Li[torch.where(hit, -s - 1, Li.shape[0] - 1)])
    if wrong == 'dead_lit':
        L = torch.where(dead[:, None], torch.ones_like(L), L)
    return L * near[:, None], dec


def estimator(pt, mat, w, L, Dd, Ds, geometry_type, wrong=''):
    """pt [P,32] (v, n, NoV read from it), mat [P,1|D,5] (metallic, roughness, albedo), w [P,D,3], L [P,D,3] ->
    rgb_lin, dl_mean, sl_mean, spec_lin [P,3], decisions   (shade_mixed: GGX D, Schlick-GGX or height-correlated Smith G, Schlick Fresnel)"""
    D = Dd + Ds
    v, n, nov = pt[:, None, 0:3], pt[:, None, 3:6], pt[:, 14:15]
    m, r, a = mat[..., 0], mat[..., 1], mat[..., 2:5]
    nw, hraw = (n * w).sum(-1), v + w
    H = F.normalize(hraw, dim=-1)
    hv, nh = (H * v).sum(-1), (n * H).sum(-1)
    hov, nol, noh = hv.clamp(0.0, 1.0), nw.clamp(0.0, 1.0), nh.clamp(0.0, 1.0)
    fc = torch.clamp(1.0 - hov, 0.0, 1.0) ** (4.0 if wrong == 'fresnel_exp4' else 5.0)
    if geometry_type == 0:
        G = M.geometry_schlick(nov, nol, r)
    else:
        G = M.geometry_ggx_smith_correlated(nov, nol.detach() if wrong == 'no_smith_dnol' else nol, r)
    dg = M.distribution_ggx(noh, r)
    diffuse = (torch.arange(D) < Dd)[None, :]
    prob = torch.where(diffuse, nol / math.pi * (Dd / D), dg * noh / (4 * hov + 1e-5) * (Ds / D))
    W = dg * G / (4 * nov * prob + (0.0 if wrong == 'no_q_eps' else 1e-5))
    F0 = 0.04 * (1 - m[..., None]) + m[..., None] * a
    Fr = F0 + (1.0 - F0) * fc[..., None]
    spec = (Fr * L * W[..., None]).sum(1) / D
    sl = (L * W[..., None]).sum(1) / D
    diff = (a * (1 - m[..., None]) * L)[:, :Dd].sum(1) / (D if wrong == 'diffuse_over_D' else Dd)
    dl = L[:, :Dd].sum(1) / Dd
    one = torch.ones_like(nw)
    dec = {'nw': (nw >= 0, nw.abs()), 'nH': (nh >= 0, nh.abs()), 'hov_hi': (hv <= 1, (1 - hv).abs()), 'noh_hi': (nh <= 1, (1 - nh).abs()),
           'nw_hi': (nw <= 1, torch.where(diffuse, one, (1 - nw).abs())), 'hv_lo': (hv >= 0, hv.abs())}
    return diff + spec, dl, sl, spec, dec


def combine_fwd(pt, dirs_, depth, slot, outer_raw, inner_raw, human_raw, hmask, n_hum, emax, imax, Dd, Ds, geometry_type, wrong=''):
    """the arrays of nero_mc_combine_fwd_h -> rgb_lin, dl_mean, sl_mean, spec_lin [P,3], decisions"""
    P_, D = pt.shape[0], Dd + Ds
    L, dec = lights(slot, depth, outer_raw, inner_raw, human_raw, hmask, n_hum, emax, imax, wrong)
    out = estimator(pt, pt[:, None, 9:14], dirs_.reshape(P_, D, 3), L.reshape(P_, D, 3), Dd, Ds, geometry_type, wrong)
    dec.update(out[4])
    return out[:4] + (dec,)


def shading_bwd(q, geometry_type, d_dl=True, wrong='', dtype=F64, sizes=False, want_wspec=True):
    """nero_mc_combine_bwd_h followed by nero_mc_dir_bwd_h as ONE autograd problem over the arrays `q` of estimator_inputs.  Leaves: mat5,
    the three raw heads, and the specular directions as a function of the roughness (their VALUE is the kernel's own input dirs; their
    derivative is that of specular_dirs).  The light-MLP input rows X_miss, X_hit (its IDE block), X_hum are functions of the directions and
    receive the cotangents dX_miss, dX_hit, dXh -- the part the MLP backward plays in the step.
    -> dict(d_mat5 [P,5] after both calls, d_outer_raw [n_miss,3], d_inner_raw [n_hit,3],
            d_human_raw [n_hum,4] | None, d_wspec [P*Ds,3] through the BRDF terms only[, sizes [P,5]: the sum over directions of the absolute
            per-direction contributions to d_mat5])"""
    c = lambda k: None if q.get(k) is None else q[k].to(dtype)
    P_, Dd, Ds = q['P'], q['Dd'], q['Ds']
    D = Dd + Ds
    pt, w_in = c('pt'), c('dirs').reshape(P_, D, 3)
    mat5 = leaf(q['pt'][:, 9:14], dtype)
    mat = mat5[:, None, :].expand(P_, D, 5).clone().detach().requires_grad_(True) if sizes else mat5[:, None, :]
    outer, inner = leaf(q['outer_raw'], dtype), leaf(q['inner_raw'], dtype)
    human = leaf(q['human_raw'], dtype) if q.get('human_raw') is not None and q['n_hum'] > 0 else None
    w_leaf = leaf(w_in[:, Dd:], dtype)
    ws = w_leaf
    if wrong != 'no_dir_bwd':
        wf = specular_dirs(pt, c('tab_s'), mat[:, -Ds:, 1] if sizes else mat[:, :, 1])
        ws = ws + (wf - wf.detach())
    w = torch.cat([w_in[:, :Dd], ws], 1)
    L, _ = lights(q['slot'], c('depth'), outer, inner, human, c('hmask'), q['n_hum'], q['emax'], q['imax'], wrong)
    rgb, dl, _, _, _ = estimator(pt, mat, w, L.reshape(P_, D, 3), Dd, Ds, geometry_type, wrong)
    shade = (rgb * c('d_rgb')).sum() + ((dl * c('d_dl')).sum() if d_dl else 0.0)
    wr = w.reshape(-1, 3)
    mi, hi = q['miss_idx'].long(), q['hit_idx'].long()
    pm = _pidx(mi, D)
    enc = (miss_rows(wr[mi], pt[pm, 29:32], q['sphere'], wrong) * c('dX_miss')).sum() if mi.numel() else 0.0
    if hi.numel():
        enc = enc + (hit_rows(wr[hi], c('pos')[hi], c('fnrm')[hi])[:, 51:123] * c('dX_hit')[:, 51:123]).sum()
    if human is not None:
        nh = q['n_hum']
        enc = enc + (human_rows(wr[mi[:nh]], pt[pm[:nh], 29:32], c('poses')[pm[:nh]])[0] * c('dXh')).sum()
    leaves = [mat, outer, inner, w_leaf] + ([human] if human is not None else [])
    g = torch.autograd.grad(shade + enc, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if x is None else x for l, x in zip(leaves, g)]
    if sizes:
        return g[0].abs().sum(1).detach()
    out = dict(d_mat5=g[0][:, 0], d_outer_raw=g[1][:, :3], d_inner_raw=g[2][:, :3], d_human_raw=g[4] if human is not None else None)
    if not want_wspec:
        return {k: (None if t is None else t.detach()) for k, t in out.items()}
    w2 = leaf(w_in[:, Dd:], dtype)                                           # d_wspec: through the BRDF terms only (the encodings' part enters in dir_bwd)
    out['d_wspec'] = torch.autograd.grad(_shade_of_w(q, geometry_type, wrong, dtype, w2), [w2])[0].reshape(-1, 3)
    return {k: (None if t is None else t.detach()) for k, t in out.items()}


def raw_head_sizes(q, geometry_type, d_dl=True):
    """float64 sizes of the terms whose signed sum a raw-head gradient row is: the row is linear in the six cotangents d_rgb[p, :], d_dl[p, :] of
    its point, each entering through non-negative factors (Fresnel, the estimator weight, albedo (1 - metallic), the light itself), so the
    sum of the absolute gradients for one cotangent at a time is the sum of the absolute terms.  A row whose colour channels above the cap
    carry nothing and whose remaining channel cancels to 1e-3 of its terms (committed: case (65, 32, 32), reference row [0, 1.1e-5, 0]) cannot
    be resolved relative to ITSELF in float32 by any implementation; the GPU tier measures a row of d_outer_raw / d_inner_raw / d_human_raw
    against the larger of its own magnitude and this size.  -> name -> [rows, 3 | 4]"""
    out = {}
    for key in ('d_rgb', 'd_dl') if d_dl else ('d_rgb',):
        # (colour channel c of a row hears only cotangent channel c; the weight column of d_human_raw sums over the channels and needs them apart)
        for ch in (range(3) if q.get('human_raw') is not None and q['n_hum'] > 0 else (slice(None),)):
            cot = torch.zeros_like(q[key])
            cot[:, ch] = q[key][:, ch]
            q1 = {**q, 'd_rgb': torch.zeros_like(q['d_rgb']), 'd_dl': torch.zeros_like(q['d_dl']), key: cot}
            b = shading_bwd(q1, geometry_type, True, want_wspec=False)
            for k in ('d_outer_raw', 'd_inner_raw'):
                out[k] = out.get(k, 0) + b[k].abs()
            if b['d_human_raw'] is not None:
                # the weight column sums dl_c (hl_c - outer_c): the human and the outer light are each an exp with its own rounding, so the
                # two are separate terms -- evaluated with the other one switched off (raw = -1e30: exp gives exactly 0)
                dark_o, dark_h = torch.full_like(q['outer_raw'], -1e30), q['human_raw'].clone()
                dark_h[:, :3] = -1e30
                for q2 in ({**q1, 'outer_raw': dark_o}, {**q1, 'human_raw': dark_h}):
                    out['d_human_raw'] = out.get('d_human_raw', 0) + shading_bwd(q2, geometry_type, True, want_wspec=False)['d_human_raw'].abs()
    return out


def _shade_of_w(q, geometry_type, wrong, dtype, w_spec):
    c = lambda k: None if q.get(k) is None else q[k].to(dtype)
    P_, Dd, Ds = q['P'], q['Dd'], q['Ds']
    pt = c('pt')
    w = torch.cat([c('dirs').reshape(P_, Dd + Ds, 3)[:, :Dd], w_spec], 1)
    human = c('human_raw') if q['n_hum'] > 0 else None
    L, _ = lights(q['slot'], c('depth'), c('outer_raw'), c('inner_raw'), human, c('hmask'), q['n_hum'], q['emax'], q['imax'], wrong)
    rgb = estimator(pt, pt[:, None, 9:14], w, L.reshape(P_, Dd + Ds, 3), Dd, Ds, geometry_type, wrong)[0]
    return (rgb * c('d_rgb')).sum()


# ---- loss glue ------------------------------------------------------------------------------------------------------------------------------
def reg_points(pts, normals, ang01, eps):
    """-> out [2P,3] = [pts ; pts + (cos(a) x + sin(a) y) eps], a = 2 pi ang01, (x, y) the tangent frame of the normalised normal; eps [P] or float"""
    n = F.normalize(normals, dim=-1)
    x = M.orthogonal_direction(n)
    y = torch.linalg.cross(n, x)
    a = (ang01 * (2 * math.pi))[:, None]
    e = eps[:, None] if torch.is_tensor(eps) else eps
    return torch.cat([pts, pts + (torch.cos(a) * x + torch.sin(a) * y) * e])


def mat_head(raw):
    """raw [n,5] -> (metallic, roughness in [0.04^2, 1], albedo(3))"""
    s = torch.sigmoid(raw)
    return torch.cat([s[:, :1], s[:, 1:2] * R_SPAN + R_MIN, s[:, 2:]], -1)


H_R_HI, H_R_LO, H_M_HI, H_M_LO = 0.98 ** 2, 0.02 ** 2, 0.98, 0.02


def mat_loss(cfg, P_, has_reg, mat, rgb_lin, dl, gt, wrong=''):
    """cfg: dict(rgb_l1, reg_mat, reg_change, reg_lambda1, hinge_weight, reg_diffuse, reg_diffuse_lambda) -> loss [4] = (total, mean loss_rgb,
    mean loss_mat_reg, mean loss_diffuse_light), rgb_pr [P,3], decisions"""
    pr = O.linear_to_srgb(rgb_lin)
    df = pr - gt
    l_rgb = df.abs().sum(-1) if cfg['rgb_l1'] else torch.sqrt((df ** 2).sum(-1) + 1e-3)
    zero = torch.zeros((), dtype=mat.dtype)
    reg, dec = zero, {'knee_rgb': (rgb_lin <= 0.0031308, (rgb_lin - 0.0031308).abs()), 'sign_df': (df >= 0, df.abs())}
    m, r = mat[:P_, 0], mat[:P_, 1]
    if cfg['reg_mat']:
        if cfg['reg_change'] and has_reg:
            d = (mat[P_:2 * P_] - mat[:P_]).abs()
            wa = 1.0 if wrong == 'reg_albedo_weight_1' else 1.0 / 3.0
            reg = ((d[:, :2].sum(-1) + d[:, 2:].sum(-1) * wa) * cfg['reg_lambda1']).mean()
        if cfg['hinge_weight'] > 0:
            hinge = torch.clamp(r - H_R_HI, min=0) + torch.clamp(H_R_LO - r, min=0) + torch.clamp(m - H_M_HI, min=0) + torch.clamp(H_M_LO - m, min=0)
            reg = reg + cfg['hinge_weight'] * (hinge.mean() if wrong == 'hinge_mean' else hinge.sum())
    l_dl = zero
    if cfg['reg_diffuse']:
        y = O.linear_to_srgb(dl)
        vv = torch.clamp(y, 0.0, 1.0)
        dv = vv - vv.mean(-1, keepdim=True)
        l_dl = (dv.abs().sum(-1) * cfg['reg_diffuse_lambda']).mean()
        dec.update(knee_dl=(dl <= 0.0031308, (dl - 0.0031308).abs()), sign_dl=(dv >= 0, dv.abs()), dl_hi=(y <= 1, (y - 1).abs()))
    l_rgb = l_rgb.mean()
    return torch.stack([l_rgb + reg + l_dl, l_rgb, reg + zero, l_dl + zero]), pr, dec


def mat_loss_bwd(cfg, P_, has_reg, mat, rgb_lin, dl, gt, grad_out=1.0, dtype=F64):
    """-> d_mat (shape of mat), d_rgb_lin [P,3], d_dl [P,3]"""
    ls = [leaf(mat, dtype), leaf(rgb_lin, dtype), leaf(dl, dtype)]
    loss = mat_loss(cfg, P_, has_reg, ls[0], ls[1], ls[2], gt.to(dtype))[0][0] * grad_out
    g = torch.autograd.grad(loss, ls, allow_unused=True)
    return [torch.zeros_like(l) if x is None else x for l, x in zip(ls, g)]


def mat_head_bwd(raw, d_mat, dtype=F64):
    r = leaf(raw, dtype)
    return vjp([mat_head(r)], [d_mat.to(dtype)], [r])[0]


# =============================================================================================================================================
# the seeded edge input sets of the GPU tier (float32)
# =============================================================================================================================================
# Margins of DERIVED boundaries, in the units of the decision's distance.  The compared quantities are dot products of unit vectors (float32
# error ~2e-7), |p| (6e-8), plane-hit coordinates of O(1) (1e-6) and sRGB values (1e-6); the margins are >= 10 x that.  Rows of class 1
# whose roughness is at its floor are exempt from noh_hi / hov_hi (their half vector lies within 1e-6 of the normal by construction: that
# closeness is the condition the class exists for).  Decisions not named here sit on DIRECT inputs (exact ties allowed).
MARGINS = {'nw': 1e-4, 'nH': 1e-4, 'hov_hi': 1e-5, 'noh_hi': 1e-5, 'nw_hi': 1e-5, 'hv_lo': 1e-4, 'dead_margin': 1e-5, 'ortho_n': 1e-3, 'ortho_r': 1e-3,
           'nov0': 1e-3, 'dz_small': 1e-5, 'dist_pos': 1e-4, 'radius': 1e-4, 'pnorm': 1e-4, 'hw_hi': 1e-3,
           'knee_rgb': 1e-5, 'knee_dl': 1e-5, 'sign_df': 1e-4, 'sign_dl': 1e-4, 'dl_hi': 1e-4}
EST_DD_DS = ((1, 1), (3, 5), (32, 31), (32, 32), (33, 32), (1, 128), (100, 93), (130, 70))
EST_P = (1, 3, 65)
EST_CASES = tuple((P_, Dd, Ds) for Dd, Ds in EST_DD_DS for P_ in EST_P)
ROW_SHAPES = ((1, 1, 0), (1, 64, 63), (1, 64, 64), (1, 65, 64), (3, 120, 80))          # (P, Dd, Ds): P*D = 1, 127, 128, 129, 200 x 3
EXTREME_KINDS = ('rough_floor', 'rough_one', 'nov_zero', 'back_facing', 'axis_normal', 'zero_normal', 'far_point')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tab(n):
    az, el = M.fibonacci_az_el(n) if n > 0 else ([], [])
    return torch.stack([torch.as_tensor(az, dtype=F32), torch.as_tensor(el, dtype=F32)], -1).reshape(n, 2)


def _rot(g):
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    return (q * torch.sign(torch.linalg.det(q))).float()


def _point_candidates(P_, g, tab_d, tab_s):
    """one candidate per point: geometry, materials, pose, class.  The pose of every fifth point looks ALONG direction 0 of the point
    (|dz| = 5e-5 <= 1e-4 in the human frame: the plane counts as not hit); a pose need not be a rotation for the kernels"""
    rnd = lambda *s: torch.randn(*s, generator=g)
    uni = lambda *s: torch.rand(*s, generator=g)
    n = F.normalize(rnd(P_, 3), dim=-1)
    t = F.normalize(torch.linalg.cross(n, rnd(P_, 3)), dim=-1)
    nov = 0.1 + 0.85 * uni(P_, 1)
    view = (n * nov + t * torch.sqrt(1 - nov * nov)) * (0.5 + uni(P_, 1))            # unnormalised, NoV in [0.1, 0.95]
    normals = n * (0.5 + 1.5 * uni(P_, 1))
    pts = F.normalize(rnd(P_, 3), dim=-1) * (0.1 + 0.75 * uni(P_, 1))
    mat5 = torch.cat([uni(P_, 1), 0.1 + 0.8 * uni(P_, 1), uni(P_, 3)], -1)
    cls = torch.zeros(P_, dtype=torch.long)
    kind = torch.full((P_,), -1, dtype=torch.long)
    for p in range(2, P_, 4):                                               # every fourth point is an extreme one, the kinds in turn
        k = (p // 4) % len(EXTREME_KINDS)
        cls[p], kind[p] = 1, k
        name = EXTREME_KINDS[k]
        if name == 'rough_floor':
            mat5[p, 1] = R_MIN
        elif name == 'rough_one':
            mat5[p, 1] = 1.0
        elif name == 'nov_zero':
            normals[p], view[p] = torch.tensor([0.0, 0.0, 2.0]), torch.tensor([0.6, -0.8, 0.0])        # v . n == 0 exactly
        elif name == 'back_facing':
            view[p] = -view[p] + 0.2 * t[p]
        elif name == 'axis_normal':
            normals[p] = torch.eye(3)[(p // 28) % 3] * (1.0 if (p // 4) % 2 else -1.0)
        elif name == 'zero_normal':
            normals[p] = 0.0
        elif name == 'far_point':
            pts[p] = F.normalize(pts[p], dim=-1) * (0.9995 + 0.001 * float(uni(1)))    # (0.999 p stays inside the unit sphere)
    poses = torch.zeros(P_, 3, 4)
    for p in range(P_):
        poses[p, :, :3] = _rot(g)
        poses[p, :, 3] = torch.tensor([0.2, -0.1, 0.3]) * rnd(3) + torch.tensor([0.0, 0.0, 0.6 if p % 2 else -0.6])
    c = dict(pts=pts, view=view, normals=normals, mat5=mat5, poses=poses, cls=cls, kind=kind, rand_d=uni(P_), rand_s=uni(P_))
    D = tab_d.shape[0] + tab_s.shape[0]
    w = dirs(point_setup(pts, view, normals, mat5, c['rand_d'], c['rand_s'])[0], tab_d, tab_s)[0].reshape(P_, D, 3)
    for p in range(1, P_, 5):
        w0 = w[p, 0].double()
        if float(w0.norm()) > 0.5:
            zax = F.normalize(torch.linalg.cross(w0, torch.tensor([0.3, 0.5, 0.8], dtype=F64)), dim=-1)
            poses[p, 2, :3] = (zax + w0 / (w0 * w0).sum() * (5e-5 if p % 2 else -5e-5)).float()
    return c


def point_decisions(c, tab_d, tab_s, dtype, sphere=True):
    """every DERIVED decision of a set of points (all D directions each), evaluated in `dtype` from the float32 arrays -> name -> (side, dist),
    leading dimension P"""
    f = lambda t: t.to(dtype)
    P_ = c['pts'].shape[0]
    Dd, Ds = tab_d.shape[0], tab_s.shape[0]
    D = Dd + Ds
    pt32 = point_setup(c['pts'], c['view'], c['normals'], c['mat5'], c['rand_d'], c['rand_s'])[0]
    dec = {k: v for k, v in point_setup(f(c['pts']), f(c['view']), f(c['normals']), f(c['mat5']), f(c['rand_d']), f(c['rand_s']))[1].items()}
    w32 = dirs(pt32, tab_d, tab_s)[0]
    pt, w = f(pt32), f(w32)
    z = torch.zeros(P_ * D, 3, dtype=dtype)
    dec.update(estimator(pt, pt[:, None, 9:14], w.reshape(P_, D, 3), z.reshape(P_, D, 3), Dd, Ds, 0)[4])
    if Ds:
        dec.update(dead_rays(pt, w, Dd, Ds, 0)[1])
    hd = human_flags(pt, w, f(c['poses']), D)[1]
    dec.update({k: (s.reshape(P_, D), d.reshape(P_, D)) for k, (s, d) in hd.items()})
    pn = torch.norm(pt[:, 29:32], dim=-1)
    dec['pnorm'] = (pn > 0.999, (pn - 0.999).abs())
    return dec


def _exempt(key, c):
    """rows a margin does not apply to: exact ties built from direct inputs, and the closeness the extreme class exists for"""
    kind = c['kind']
    name = lambda s: kind == EXTREME_KINDS.index(s)
    if key in ('noh_hi', 'hov_hi', 'nw_hi'):
        return name('rough_floor') | name('zero_normal')
    if key in ('nw', 'nH', 'dead_margin', 'hv_lo'):
        return name('zero_normal')
    if key == 'ortho_n':                                                     # (n = +-e_x: both candidates have length 1 exactly, in any precision)
        return name('zero_normal') | name('axis_normal')
    if key == 'nov0':
        return name('nov_zero') | name('zero_normal')
    return torch.zeros_like(kind, dtype=torch.bool)


def margins_ok(dec, c):
    """[P] bool: every derived decision of the point at least its margin away from the boundary"""
    ok = torch.ones(c['pts'].shape[0], dtype=torch.bool)
    for key, (_, dist) in dec.items():
        if key in MARGINS:
            d = dist.reshape(dist.shape[0], -1).min(-1)[0] >= MARGINS[key]
            ok &= d | _exempt(key, c)
    return ok


@functools.lru_cache(maxsize=None)
def point_inputs(P_, Dd, Ds, seed=0):
    """P points whose every direction is clear of every derived boundary: candidates are drawn per attempt and a point keeps its first
    candidate that passes (seeded, so the set is fixed) -> dict(pts, view, normals, mat5, poses, cls, kind, rand_d, rand_s, tab_d, tab_s)"""
    tab_d, tab_s = _tab(Dd), _tab(Ds)
    out, todo = None, torch.ones(P_, dtype=torch.bool)
    for attempt in range(40):
        c = _point_candidates(P_, _gen(7000 + 131 * P_ + 17 * Dd + Ds + 1009 * attempt + seed), tab_d, tab_s)
        ok = margins_ok(point_decisions(c, tab_d, tab_s, F64), c)
        if out is None:
            out = {k: v.clone() for k, v in c.items()}
        take = todo & ok
        for k in out:
            out[k][take] = c[k][take]
        todo &= ~ok
        if not bool(todo.any()):
            break
    assert not bool(todo.any()), 'a point found no candidate clear of every margin in 40 attempts'
    out.update(tab_d=tab_d, tab_s=tab_s)
    return out


@functools.lru_cache(maxsize=None)
def estimator_inputs(P_, Dd, Ds, human=1, sphere=0, n_hum_mode='some'):
    """_estimator_inputs with the first seed (0, 1, ...) at which, with the human light on and n_hum_mode 'some', the human-light MLP owns
    some but not all miss rows (0 < n_hum < n_miss): at P = 1 with two directions that takes a few draws"""
    for seed in range(200):
        q = _estimator_inputs(P_, Dd, Ds, human, sphere, n_hum_mode, seed)
        if not human or n_hum_mode != 'some' or 0 < q['n_hum'] < q['miss_idx'].numel():
            return q
    raise AssertionError('no seed gives 0 < n_hum < n_miss')


def _estimator_inputs(P_, Dd, Ds, human, sphere, n_hum_mode, seed):
    """the arrays of the estimator entry points for P points with Dd + Ds directions.  pt and dirs are the float32 CPU evaluation of
    point_setup / dirs; depth, hit positions and face normals stand in for the tracer; slot / miss_idx / hit_idx / n_hum come from `split`.
    Direct inputs sit exactly ON their boundaries (depth == 1e-5 and == 10, raw head == its cap, hmask in {0, 1} and, so that the clamp of
    the human weight is reached from both sides, 2 and -0.5).  With P >= 8 point P-3 has only misses, P-2 only hits and every ray
    of P-1 is dead (the slot is an input); n_hum_mode: 'some' (the split's own count), 'none' (0) or 'all' (every miss row)"""
    c = point_inputs(P_, Dd, Ds, seed)
    g = _gen(9000 + 131 * P_ + 17 * Dd + Ds + 5 * human + sphere + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    uni = lambda *s: torch.rand(*s, generator=g)
    D, N = Dd + Ds, P_ * (Dd + Ds)
    pt = point_setup(c['pts'], c['view'], c['normals'], c['mat5'], c['rand_d'], c['rand_s'])[0].contiguous()
    w, orig = dirs(pt, c['tab_d'], c['tab_s'])
    w = w.contiguous()
    u = uni(N)
    depth = torch.where(u < 0.45, 0.05 + 3.0 * uni(N), torch.full((N,), 1e10))
    edge = torch.tensor([1e-5, 10.0, 0.0, 1.0000001e-5, 9.999999])
    if N >= 16:
        depth[torch.arange(5) * (N // 5) + 1] = edge                         # on / just beside depth == 1e-5 and depth == 10
    dead = dead_rays(pt, w, Dd, Ds, 0)[0]
    if P_ >= 8:
        depth.reshape(P_, D)[P_ - 3] = 1e10
        depth.reshape(P_, D)[P_ - 2] = 0.5 + uni(D)
        dead.reshape(P_, D)[P_ - 1] = True
    hum = human_flags(pt, w, c['poses'], D)[0] if human else None
    slot, miss_idx, hit_idx, n_hum = split(depth, dead, hum)
    n_miss, n_hit = miss_idx.numel(), hit_idx.numel()
    if human:
        n_hum = {'some': n_hum, 'none': 0, 'all': n_miss}[n_hum_mode]
    emax, imax = 1.0, 0.5
    outer_raw, inner_raw = torch.full((n_miss, 4), 77.0), torch.full((n_hit, 4), 77.0)
    outer_raw[:, :3], inner_raw[:, :3] = 1.2 * rnd(n_miss, 3), 1.2 * rnd(n_hit, 3)
    if n_miss > 4:
        outer_raw[1, 0], outer_raw[2, 1] = emax, emax + 2.0
    if n_hit > 4:
        inner_raw[1, 2], inner_raw[3, 0] = imax, imax + 1.5
    human_raw = hmask = dXh = None
    if human:
        human_raw = 0.8 * rnd(n_hum, 4)
        human_raw[:, 3] = torch.where(human_raw[:, 3].abs() < 2e-3, torch.full((n_hum,), -0.01), human_raw[:, 3])   # (hw_hi: clear of 1, or exactly on it)
        hmask = human_rows(w[miss_idx[:n_hum].long()], pt[_pidx(miss_idx[:n_hum], D), 29:32], c['poses'][_pidx(miss_idx[:n_hum], D)])[1] \
            if n_hum else torch.zeros(0)
        if n_hum > 6:
            human_raw[0, 3], human_raw[1, 0] = 0.0, 0.0
            hmask[2], human_raw[2, 3] = 2.0, -2.0                                # weight 2 e^-2 = 0.27: inside the clamp
            hmask[3], human_raw[3, 3] = 2.0, -0.1                                # weight 1.81: above 1, clamped, no gradient
            hmask[4], human_raw[4, 3] = -0.5, -0.3                               # weight -0.37: below 0, clamped
            hmask[5] = 0.0                                                       # an owned row that is masked out: no light, no gradient
        dXh = rnd(n_hum, 24)
    fn = F.normalize(rnd(N, 3), dim=-1) * (0.5 + uni(N, 1))
    return dict(P=P_, Dd=Dd, Ds=Ds, sphere=sphere, seed=seed, cls=c['cls'], kind=c['kind'], pt=pt, dirs=w, orig=orig, tab_d=c['tab_d'], tab_s=c['tab_s'],
                poses=c['poses'], depth=depth, dead=dead, hum=hum, slot=slot, miss_idx=miss_idx, hit_idx=hit_idx, n_hum=n_hum if human else 0,
                outer_raw=outer_raw, inner_raw=inner_raw, human_raw=human_raw, hmask=hmask, emax=emax, imax=imax,
                pos=0.6 * rnd(N, 3), fnrm=fn, d_rgb=rnd(P_, 3), d_dl=rnd(P_, 3), dX_miss=rnd(n_miss, 144 if sphere else 72),
                dX_hit=rnd(n_hit, 128), dXh=dXh)


LOSS_P = (1, 255, 256, 257, 513, 65537)


def _reg_eps(P_, g):
    """step sizes of the tangent-plane perturbation: |eps| in [0.01, 0.2] with both signs (the step is judged against its own size, so a
    step of 1e-6 would set the float32 floor of every row), and every 97th exactly zero: that row is a copy, judged exactly"""
    e = (0.01 + 0.05 * torch.randn(P_, generator=g).abs().clamp(max=3.8)) * torch.where(torch.rand(P_, generator=g) < 0.5, -1.0, 1.0)
    e[5::97] = 0.0
    return e


@functools.lru_cache(maxsize=None)
def loss_inputs(P_, seed=0):
    """mat [2P,5] (rows P.. the materials at the perturbed points), rgb_lin, dl, gt [P,3], raw [P,5], d_mat [P,5].  Roughness / metallic sit
    within four float32 steps of the four hinge thresholds, on both sides (direct inputs); materials of some perturbed points equal the point's own
    (|0|); the sRGB knee, the sign of pr - gt, the sign of v - mean(v) and the clamp of the diffuse light are DERIVED: clear by MARGINS"""
    g = _gen(11000 + P_ + seed)
    uni = lambda *s: torch.rand(*s, generator=g)
    mat = uni(2 * P_, 5)
    mat[P_:] = (mat[:P_] + 0.1 * torch.randn(P_, 5, generator=g)).clamp(0.0, 1.0)
    same = torch.arange(P_) % 5 == 3
    mat[P_:][same] = mat[:P_][same]
    # (none of the four thresholds is a float32 number: the kernel and float32 torch compare with the ROUNDED constant, float64 with the exact
    #  one, so a row exactly on the rounded constant has no common answer; rows sit four float32 steps on either side of it instead)
    th = torch.tensor([H_R_HI, H_R_LO, H_M_HI, H_M_LO], dtype=F64).float()
    if P_ > 16:
        for j, (col, t) in enumerate(((1, th[0]), (1, th[1]), (0, th[2]), (0, th[3]))):
            mat[3 * j, col], mat[3 * j + 1, col], mat[3 * j + 2, col] = t * (1 + 4.8e-7), t * (1 - 4.8e-7), t + 0.015
    rgb_lin = uni(P_, 3) ** 3 * 1.6
    dl = uni(P_, 3) ** 2 * 1.4
    dark = torch.arange(P_) % 7 == 2
    rgb_lin[dark], dl[dark] = rgb_lin[dark] * 1e-3, dl[dark] * 1e-3
    if P_ > 16:
        dl[13], dl[14], dl[15] = torch.tensor([1.0, 0.3, 0.2]), torch.tensor([1.5, 2.0, 3.0]), 0.0      # y == 1 (tie), all clamped, all zero
    for t in (rgb_lin, dl):
        t[(t - 0.0031308).abs() < 10 * MARGINS['knee_rgb']] = 0.004
    for _ in range(8):                                                       # v - mean(v) and y - 1 clear of zero (or exactly zero: rows 14, 15)
        y = O.linear_to_srgb(dl.double())
        v = y.clamp(0.0, 1.0)
        dv = (v - v.mean(-1, keepdim=True)).abs()
        bad = (((dv < 3 * MARGINS['sign_dl']) & (dv != 0)) | (((y - 1).abs() < 3 * MARGINS['dl_hi']) & (y != 1))).any(-1)
        if not bool(bad.any()):
            break
        dl[bad] = torch.tensor([0.12, 0.35, 0.7])                            # (a triple clear of everything)
    assert not bool(bad.any())
    pr = O.linear_to_srgb(rgb_lin.double())
    off = (1e-3 + 0.5 * uni(P_, 3)) * torch.where(uni(P_, 3) < 0.5, -1.0, 1.0)
    gt = (pr + off).float()
    return dict(mat=mat, rgb_lin=rgb_lin, dl=dl, gt=gt, raw=3 * torch.randn(P_, 5, generator=g), d_mat=torch.randn(2 * P_, 5, generator=g),
                pts=torch.randn(P_, 3, generator=g), normals=torch.randn(P_, 3, generator=g), ang01=uni(P_), eps=_reg_eps(P_, g))


LOSS_CFGS = tuple(dict(rgb_l1=a, reg_mat=b, reg_change=c_, reg_lambda1=0.005, hinge_weight=h, reg_diffuse=d, reg_diffuse_lambda=0.1, has_reg=r)
                  for a, b, c_, h, d, r in ((0, 1, 1, 1.0, 1, 1), (1, 1, 1, 0.0, 1, 1), (0, 1, 0, 2.0, 0, 1), (1, 0, 1, 1.0, 1, 1), (0, 1, 1, 2.0, 1, 0),
                                            (1, 1, 0, 0.0, 0, 0)))
