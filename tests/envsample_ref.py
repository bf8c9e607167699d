"""Plain torch / numpy restatement of the light table, its inversion, its density and the MIS estimator (nero_amd/csrc/envsample.hip,
include/nero_hip_envsample.h), dtype-generic where the kernel computes in float32: one source serves float64 and float32.  The integer part
-- weights from given float weights, running sum, inversion -- is integers and float64 only, as on the device, and is compared bit for bit.
Reuses tests/relight_ref.py (env_lookup, proper_map, sample_table, floors_and_errors, occluded, scene, ROT, MARGIN) and tests/mc_shade_ref.py
(the record, the directions of the two BRDF strategies, the dead rule)."""
import math

import numpy as np
import torch

from tests import mc_shade_ref as R
from tests import relight_ref as RR
from tests.relight_ref import MARGIN, ROT, env_lookup, floors_and_errors, occluded, proper_map, sample_table, scene  # noqa: F401

F32, F64 = torch.float32, torch.float64
ONE_BELOW = 1.0 - 2.0 ** -24
MAX_WEIGHT_BITS, TOTAL_BITS = 40, 62
STENCIL = (0.0, 0.5, 1.0)            # positions inside a cell, along each axis, at which the table reads the map


def _pi(dt):
    """the kernel's constants are float32 values; float64 takes the exact ones"""
    return (float(np.float32(math.pi)), float(np.float32(2 * math.pi))) if dt == F32 else (math.pi, 2 * math.pi)


# ---- the grid -------------------------------------------------------------------------------------------------------------------------------
def grid_dir(u, v):
    """(u, v) -> direction [.,3], cos(elevation); dtype of u rules"""
    PI, TWO_PI = _pi(u.dtype)
    el, phi = (v - 0.5) * PI, (u - 0.5) * TWO_PI
    ce = torch.cos(el)
    return torch.stack([-(ce * torch.cos(phi)), ce * torch.sin(phi), torch.sin(el)], -1), ce


def cell_centres(gh, gw, dtype=F64):
    """-> directions [gh gw,3], max(cos el, 0) [gh gw] of the cell centres, row-major"""
    r, c = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing='ij')
    u = (c.reshape(-1).to(dtype) + 0.5) / torch.tensor(float(gw), dtype=dtype)
    v = 1.0 - (r.reshape(-1).to(dtype) + 0.5) / torch.tensor(float(gh), dtype=dtype)
    d, ce = grid_dir(u, v)
    return d, torch.clamp(ce, min=0.0)


def weights(env, convention, rot=None, clamp=0.0, dtype=F64):
    """a [gh gw] in `dtype`: luminance of env_lookup at the cell centres x cos el; not finite or negative -> 0.  -> a, fallback (bool): no
    cell has a weight, a = cos el instead"""
    gh, gw = env.shape[:2]
    _, ce = cell_centres(gh, gw, dtype)
    r, c = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing='ij')
    r, c = r.reshape(-1).to(dtype), c.reshape(-1).to(dtype)
    lum = lambda k: torch.tensor(k, dtype=F32).to(dtype)
    best = torch.zeros_like(ce)
    for t in STENCIL:                                           # corners, edge midpoints and centre of the cell: the largest luminance
        for s in STENCIL:
            u = (c + s) / torch.tensor(float(gw), dtype=dtype)
            v = 1.0 - (r + t) / torch.tensor(float(gh), dtype=dtype)
            L, _ = env_lookup(env, grid_dir(u, v)[0], convention, rot, clamp)
            y = (lum(0.2126) * L[:, 0] + lum(0.7152) * L[:, 1]) + lum(0.0722) * L[:, 2]
            best = torch.maximum(best, torch.where(torch.isfinite(y) & (y > 0), y, torch.zeros_like(y)))
    y = best * ce
    a = torch.where(torch.isfinite(y) & (y > 0), y, torch.zeros_like(y))
    if not bool((a > 0).any()):
        return ce, True
    return a, False


def weight_bits(N):
    L = int(N - 1).bit_length()
    return min(MAX_WEIGHT_BITS, TOTAL_BITS - L)


def table_from_weights(a, fallback=False):
    """a: float32 weights [N] (numpy; the fallback's when it was taken) -> cdf [N] int64, info [5] int64 = (total, zero cells, e, B, fallback)"""
    a = np.asarray(a, np.float32).astype(np.float64)
    N = a.shape[0]
    B = weight_bits(N)
    mx = float(a.max())
    e = 0 if (fallback or not mx > 0) else int(math.frexp(mx)[1])
    w = np.floor(np.ldexp(a, B - e)).astype(np.int64)
    cdf = np.cumsum(w, dtype=np.int64)
    return cdf, np.asarray([cdf[-1], int((w == 0).sum()), e, B, int(fallback)], np.int64)


# ---- inversion, density ---------------------------------------------------------------------------------------------------------------------
def frac_shift(tab, shift):
    """frac(tab + shift) capped at 1 - 2^-24, in float32 as the kernel: tab [Dl], shift [P] or None -> [P,Dl] float32 numpy"""
    t = np.asarray(tab, np.float32)[None, :]
    s = t + (np.float32(0) if shift is None else np.asarray(shift, np.float32)[:, None])
    s = s.astype(np.float32)
    return np.minimum(np.maximum(s - np.floor(s), np.float32(0)), np.float32(ONE_BELOW)).astype(np.float32)


def draw(cdf, gh, gw, u1, u2):
    """the header's A LIGHT SAMPLE in integers and float64: cdf [gh gw] int64 numpy, u1, u2 float32 arrays of one shape ->
    row, col (int64), x1, x2 (float64, clamped to [0, 1 - 2^-24]), w_cell (int64)"""
    cdf = np.asarray(cdf, np.int64)
    total = int(cdf[-1])
    Rm = cdf.reshape(gh, gw)[:, -1]
    shp = np.shape(u1)
    u1, u2 = np.asarray(u1, np.float32).reshape(-1).astype(np.float64), np.asarray(u2, np.float32).reshape(-1).astype(np.float64)
    s1 = u1 * np.float64(total)
    t1 = np.minimum(s1.astype(np.int64), total - 1)
    row = np.searchsorted(Rm, t1, side='right').astype(np.int64)                    # the first r with R_r > t1
    base = np.where(row > 0, Rm[np.maximum(row - 1, 0)], 0).astype(np.int64)
    rowtot = Rm[row] - base
    x1 = np.clip((s1 - base.astype(np.float64)) / rowtot.astype(np.float64), 0.0, ONE_BELOW)
    s2 = u2 * rowtot.astype(np.float64)
    t2 = base + np.minimum(s2.astype(np.int64), rowtot - 1)
    k = np.searchsorted(cdf, t2, side='right').astype(np.int64)                     # cdf[row gw - 1] = base <= t2 < R_row: k lies in the row
    col = k - row * gw
    prev = np.where(k > 0, cdf[np.maximum(k - 1, 0)], 0).astype(np.int64)
    wc = cdf[k] - prev
    x2 = np.clip((s2 - (prev - base).astype(np.float64)) / wc.astype(np.float64), 0.0, ONE_BELOW)
    return tuple(z.reshape(shp) for z in (row, col, x1, x2, wc))


def pdf_light(cdf, gh, gw, cell, v):
    """p_l of the cells `cell` (int64 numpy / tensor) for grid coordinates v (tensor; its dtype rules)"""
    cdf = np.asarray(cdf, np.int64)
    k = np.asarray(cell, np.int64)
    wc = cdf[k] - np.where(k > 0, cdf[np.maximum(k - 1, 0)], 0)
    dt = v.dtype
    PI, TWO_PI = _pi(dt)
    pc = torch.from_numpy(wc.astype(np.float64) / np.float64(int(cdf[-1]))).to(dt)  # (float32: the rounding of the float64 quotient)
    ce = torch.clamp(torch.cos((v - 0.5) * PI), min=1e-6)
    t = lambda x: torch.tensor(float(x), dtype=dt)
    if dt == F32:
        return (pc * (t(gh) * t(gw))) / ((torch.tensor(TWO_PI, dtype=dt) * torch.tensor(PI, dtype=dt)) * ce)
    return pc * (gh * gw) / (2 * math.pi ** 2 * ce)


def lookup_cell(d, gh, gw):
    """cell of a direction another strategy drew -> cell [n] int64 numpy, v [n] (dtype of d), margin [n]: the distance of the direction, in
    (u, v) units, from the nearest cell border it could cross, or from the grid's axis where u is ill-conditioned"""
    dt = d.dtype
    PI, TWO_PI = _pi(dt)
    ax = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    u = torch.atan2(d[:, 1], -d[:, 0]) / TWO_PI + 0.5
    v = torch.atan2(d[:, 2], ax) / PI + 0.5
    y, x = (1.0 - v) * gh, u * gw
    row = torch.clamp(torch.floor(y), 0, gh - 1).long()
    col = torch.clamp(torch.floor(x), 0, gw - 1).long()
    dy = (y - torch.round(y)).abs() / gh
    dx = (x - torch.round(x)).abs() / gw
    dy = torch.where((torch.round(y) <= 0) | (torch.round(y) >= gh) | (gh == 1), torch.ones_like(dy), dy)     # the clamped ends are no border
    dx = torch.where(torch.tensor(gw == 1), torch.ones_like(dx), dx)
    pole = ax / torch.clamp(torch.norm(d, dim=-1), min=1e-30)
    pole = torch.where(torch.tensor(gw == 1), torch.ones_like(pole), pole)
    margin = torch.minimum(torch.minimum(dx, dy), pole)
    margin = torch.where(torch.norm(d, dim=-1) == 0, torch.ones_like(margin), margin)     # the zero vector: a tie of direct inputs, exact
    return (row * gw + col).numpy(), v, margin


def mis_rays(pt, tab_d, tab_s, tab_l, rand_l, cdf, gh, gw, geometry_type):
    """the sample set of nero_relight_mis_rays in the dtype of pt: pt [P,32], tables [.,2], rand_l [P,2] float32 or None, cdf numpy int64 ->
    w, o [P D,3], dead [P D] bool, cell [P D] int64 numpy, pdf_l [P D], margin [P D] (1 for light samples: their cell is exact), is_light"""
    dt = pt.dtype
    P_, Dd, Ds, Dl = pt.shape[0], tab_d.shape[0], tab_s.shape[0], tab_l.shape[0]
    D = Dd + Ds + Dl
    wb, _ = R.dirs(pt, tab_d.to(dt), tab_s.to(dt))
    wb = wb.reshape(P_, Dd + Ds, 3)
    tl = tab_l.float().numpy()
    u1 = frac_shift(tl[:, 0], None if rand_l is None else rand_l[:, 0].float().numpy())
    u2 = frac_shift(tl[:, 1], None if rand_l is None else rand_l[:, 1].float().numpy())
    u1, u2 = np.broadcast_to(u1, (P_, Dl)), np.broadcast_to(u2, (P_, Dl))
    row, col, x1, x2, _ = draw(cdf, gh, gw, u1, u2)
    as_t = lambda z: torch.from_numpy(np.ascontiguousarray(z))
    x1, x2 = as_t(x1), as_t(x2)
    if dt == F32:
        x1, x2 = x1.float(), x2.float()
    gwt, ght = torch.tensor(float(gw), dtype=dt), torch.tensor(float(gh), dtype=dt)
    u = (as_t(col).to(dt) + x2) / gwt
    v = 1.0 - (as_t(row).to(dt) + x1) / ght
    wl, _ = grid_dir(u.reshape(-1), v.reshape(-1))
    w = torch.cat([wb, wl.reshape(P_, Dl, 3)], 1)
    o = pt[:, None, 29:32] + w * 1e-5
    cell_b, v_b, margin_b = lookup_cell(wb.reshape(-1, 3), gh, gw)
    cell = np.concatenate([cell_b.reshape(P_, Dd + Ds), row * gw + col], 1)
    vv = torch.cat([v_b.reshape(P_, Dd + Ds), v], 1)
    pdf = pdf_light(cdf, gh, gw, cell.reshape(-1), vv.reshape(-1))
    nw = (pt[:, None, 3:6] * w).sum(-1)
    later = (torch.arange(D) >= Dd)[None, :]
    dead = later & (nw < -1e-6) & (geometry_type == 0)
    margin = torch.cat([margin_b.reshape(P_, Dd + Ds), torch.ones(P_, Dl, dtype=margin_b.dtype)], 1)
    is_light = (torch.arange(D) >= Dd + Ds)[None, :].expand(P_, D)
    return w.reshape(-1, 3), o.reshape(-1, 3), dead.reshape(-1), cell.reshape(-1), pdf, margin.reshape(-1), is_light.reshape(-1)


# ---- the estimator --------------------------------------------------------------------------------------------------------------------------
def brdf_terms(pt, w, geometry_type):
    """pt [P,32], w [P,D,3] -> nol, nov, dg, G, fc, p_code, p_act (the saturations and formulas of brdf_weight; p_code = D_ggx NoH / (4 HoV +
    1e-5) is the density the estimators divide a GGX sample by, p_act = D(w.r) w.r the density the GGX sampler has)"""
    v, n, nov = pt[:, None, 0:3], pt[:, None, 3:6], pt[:, 14:15]
    r = pt[:, 10:11]
    hraw = v + w
    H = hraw / torch.clamp(torch.sqrt((hraw * hraw).sum(-1, keepdim=True)), min=1e-12)
    hov, nol, noh = (H * v).sum(-1).clamp(0.0, 1.0), (n * w).sum(-1).clamp(0.0, 1.0), (n * H).sum(-1).clamp(0.0, 1.0)
    fc = torch.clamp(1.0 - hov, 0.0, 1.0) ** 5
    a2 = r * r
    if geometry_type == 0:
        k = r * 0.5
        G = (nov / (nov * (1 - k) + k + 1e-5)) * (nol / (nol * (1 - k) + k + 1e-5))
    else:
        cv2, cl2 = nov * nov, nol * nol
        G = 2.0 / (torch.sqrt(1 + a2 * ((1 - cv2) / (cv2 + 1e-7))) + torch.sqrt(1 + a2 * ((1 - cl2) / (cl2 + 1e-7))))
    t = noh * noh * (a2 - 1.0) + 1.0
    PI = _pi(pt.dtype)[0]
    dg = a2 / (PI * t * t + 1e-4)
    pcode = dg * noh / (4 * hov + 1e-5)
    cr = (pt[:, None, 6:9] * w).sum(-1).clamp(0.0, 1.0)
    tr = cr * cr * (a2 - 1.0) + 1.0
    pact = a2 / torch.clamp(PI * tr * tr, min=1e-30) * cr
    return nol, nov, dg, G, fc, pcode, pact


def mis_estimator(pt, w, L, pdf_l, Dd, Ds, Dl, geometry_type):
    """pt [P,32], w, L [P,D,3], pdf_l [P,D] -> rgb_lin, diffuse_lin, spec_lin [P,3]: every sample weighed by the mixture of the densities
    the three samplers HAVE; the specular integrand carries S(w) = 1 + p_act / (p_code + 1e-5) (the header says why)"""
    D = Dd + Ds + Dl
    PI = _pi(pt.dtype)[0]
    nol, nov, dg, G, fc, pcode, pact = brdf_terms(pt, w, geometry_type)
    pd = nol / PI
    pmix = ((Dd * pd + Ds * pact) + Dl * pdf_l) / D
    dterm = torch.where((nol > 0) & (pmix > 0), pd / torch.where(pmix > 0, pmix, torch.ones_like(pmix)), torch.zeros_like(pd))
    S = 1.0 + pact / (pcode + 1e-5)
    W = S * dg * G / (4 * nov * pmix + 1e-5)
    m, alb = pt[:, None, 9:10], pt[:, None, 11:14]
    F0 = 0.04 * (1 - m) + m * alb
    Fr = F0 + (1.0 - F0) * fc[..., None]
    spec = (Fr * L * W[..., None]).sum(1) / D
    diff = (alb * (1 - m) * L * dterm[..., None]).sum(1) / D
    return diff + spec, diff, spec


def relight_mis(pt, w, blocked, dead, pdf_l, env, convention, rot, clamp, Dd, Ds, Dl, geometry_type):
    """-> rgb_lin, diffuse_lin, spec_lin [P,3]: mis_estimator with L = the environment's radiance where the shadow ray is free and the
    sample not dead, else 0"""
    P_, D = pt.shape[0], Dd + Ds + Dl
    L, _ = env_lookup(env, w, convention, rot, clamp)
    L = torch.where((blocked | dead)[:, None], torch.zeros_like(L), L)
    return mis_estimator(pt, w.reshape(P_, D, 3), L.reshape(P_, D, 3), pdf_l.reshape(P_, D), Dd, Ds, Dl, geometry_type)


# ---- quadrature -----------------------------------------------------------------------------------------------------------------------------
def integrals(pt, env, convention, geometry_type, n):
    """the expectation of the two-strategy estimator at the points pt [P,32] (float64) under an unoccluded map, term by term, by midpoint
    quadrature over an n x 2n grid in (cos theta, phi) of the world sphere.  With f = F L D_ggx G / (4 NoV), the integrand as the estimators
    state it:
      I_diff = albedo (1 - m) Int L NoL / pi dw        the cosine samples' diffuse mean
      I_cos  = Int f dw                                the cosine samples' specular half: each f / p_d, and p_d IS their density
      I_ggx  = Int f p_act / (p_code + 1e-5) dw        the GGX samples' half: each f / p_code, drawn with density p_act
    p_code = D_ggx NoH / (4 HoV + 1e-5) is the density shade_mixed divides by, p_act = D(w.r) w.r with D(c) = a^2 / (pi (c^2 (a^2 - 1) + 1)^2)
    the density its sampler has (a GGX lobe laid around the reflection r itself).  -> I_diff, I_cos, I_ggx [P,3]"""
    phi = (torch.arange(2 * n, dtype=F64) + 0.5) / (2 * n) * (2 * math.pi)
    dw = 4 * math.pi / (2 * n * n)
    m, alb = pt[:, 9:10], pt[:, 11:14]
    F0 = (0.04 * (1 - m) + m * alb)[:, None]
    I_d, I_s, I_t = (torch.zeros(pt.shape[0], 3, dtype=F64) for _ in range(3))
    rows = max(1, (1 << 18) // (2 * n))                                               # a quarter of a million directions at a time
    for r0 in range(0, n, rows):
        z = (torch.arange(r0, min(r0 + rows, n), dtype=F64) + 0.5) / n * 2 - 1
        zz, pp = torch.meshgrid(z, phi, indexing='ij')
        s = torch.sqrt(1 - zz * zz)
        d = torch.stack([s * torch.cos(pp), s * torch.sin(pp), zz], -1).reshape(-1, 3)
        L, _ = env_lookup(env, d, convention)
        nol, nov, dg, G, fc, pcode, pact = brdf_terms(pt, d[None], geometry_type)
        Fr = F0 + (1.0 - F0) * fc[..., None]
        f = Fr * L[None] * (dg * G / (4 * nov))[..., None]
        I_d += (alb * (1 - m)) * ((nol / math.pi)[..., None] * L[None]).sum(1) * dw
        I_s += f.sum(1) * dw
        I_t += (f * (pact / (pcode + 1e-5))[..., None]).sum(1) * dw
    return I_d, I_s, I_t


# ---- the committed cases of the sample-set and fused tests -----------------------------------------------------------------------------------
# one lane of each kind, exactly one wavefront, one sample past a wavefront, a lone light sample, several wavefronts
MIS_CASES = ((1, 1, 1), (16, 16, 32), (3, 2, 60), (40, 24, 1), (96, 160, 200))
MIS_P = (1, 5, 300)


def env_of_case(i):
    """(map, convention, rotation, cap) as tests/test_relight_gpu.py's _env_of_case: the conventions in turn, every other case rotated, every
    third capped, a texel at 1000 x"""
    conv = i % 3
    return proper_map(16, 32, seed=i, hot=(5, 9, 1000.0)), conv, (ROT if i % 2 else None), (50.0 if i % 3 == 1 else None)


def candidates(P_, Dd, Ds, Dl):
    """mc_shade_ref's point candidates (every fourth an extreme one), moved outside the sphere of relight_ref.scene so that part of their
    rays is blocked, with the light samples' shifts rand_l [P,2] -> dict, tab_d, tab_s, tab_l (float32)"""
    tab_d, tab_s, tab_l = sample_table(Dd), sample_table(Ds), sample_table(Dl)
    g = torch.Generator().manual_seed(900 + 7 * P_ + 13 * Dd + 5 * Ds + Dl)
    c = R._point_candidates(P_, g, tab_d, tab_s)
    c['pts'] = torch.nn.functional.normalize(c['pts'], dim=-1) * (0.52 + 0.3 * torch.rand(P_, 1, generator=g))
    c['rand_l'] = torch.rand(P_, 2, generator=g)
    return c, tab_d, tab_s, tab_l
