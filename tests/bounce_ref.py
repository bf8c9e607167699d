"""Plain torch / numpy restatement of the relighter's one bounce (nero_amd/csrc/relight_estimator.hip, include/nero_hip_bounce.h), dtype-generic:
one source serves float64 and float32.  It stands on tests/relight_ref.py (closest_hit, occluded, interpolate, env_lookup), tests/
envsample_ref.py (draw, pdf_light, lookup_cell, brdf_terms, mis_estimator) and tests/mc_shade_ref.py (point_setup, estimator); what it adds
is the counter hash, the choice of the strategy, the surface record at the hit, the per-lane secondary direction and L_o.

Lanes are rows p D + j as in the kernels.  The discrete facts of a lane -- state (0 primary ray free, 1 primary sample dead, 2 bounced, 3
bounced with a dead secondary, 4 bad face), hit face, strategy, whether the second shadow ray is blocked -- are INPUTS of bounce(): facts()
makes them by brute force for the CPU tier, the GPU tier takes them from the device.  Decisions (`dec`: name -> (side, distance)) are
reported the way relight_ref.exempt reads them, per point [P, .]:
  'strategy'      the first variate against c_d and c_d + c_s;   'dead2' the secondary's dead rule (n2.w2 against -1e-6)
  'flip'          the flat normal's side of the incoming ray;     'ortho_n2' / 'ortho_r2' the tie in a frame's choice at y
  'cell2'         the looked-up cell of a secondary direction (MIS variant);  'hit' / 'shadow2' the brute-force walks (facts() only)
bounce() also returns the part of the indirect term that comes from the secondary's DIFFUSE term alone (and from its specular term alone):
the closed forms of the CPU tier need them, the kernel has no such output."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import envsample_ref as ER
from tests import mc_shade_ref as R
from tests import relight_ref as RR

F32, F64 = torch.float32, torch.float64
FREE, DEAD, BOUNCED, BOUNCED_DEAD, BAD_FACE = 0, 1, 2, 3, 4
# decisions the kernel takes in floating point and does not report; then those nero_relight_bounce_rays reports (the dead flags through the
# state, the cell, the strategy -- which is exact in float32 anyway) and those of the walks: the GPU tier takes all of these from the device
# and exempts nothing for them
CONTINUOUS_KEYS = ('pole', 'seam', 'flip', 'ortho_n2', 'ortho_r2')
EXEMPT_KEYS = CONTINUOUS_KEYS + ('strategy', 'dead_margin', 'dead2', 'cell2', 'shadow', 'hit', 'shadow2')


# ---- the hash, the strategy -----------------------------------------------------------------------------------------------------------------
def lowbias32(x):
    """numpy uint64 holding uint32 values"""
    m = np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def variates(key, D):
    """key [P] (any integers, taken mod 2^32) -> u1, u2, u3 float32 numpy [P, D]"""
    m = np.uint64(0xffffffff)
    key = (np.asarray(key).astype(np.int64) & 0xffffffff).astype(np.uint64)[:, None]
    j = np.arange(D, dtype=np.uint64)[None, :]
    k1 = lowbias32((key + j * np.uint64(0x9E3779B9)) & m)
    k2 = lowbias32((k1 + np.uint64(0x68E31DA4)) & m)
    k3 = lowbias32((k2 + np.uint64(0x68E31DA4)) & m)
    f = lambda k: ((k >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return f(k1), f(k2), f(k3)


def strategy(u1, Dd, Ds, Dl):
    """the header's choice in float32, exactly: 0 cosine, 1 GGX, 2 light (never without Dl) -> s int64 numpy, margin float64 numpy"""
    D = np.float32(Dd + Ds + Dl)
    cd, cs = np.float32(Dd) / D, np.float32(Ds) / D
    edge = np.float32(cd + cs)
    u1 = np.asarray(u1, np.float32)
    s = np.where(u1 < cd, 0, np.where((Dl == 0) | (u1 < edge), 1, 2)).astype(np.int64)
    margin = np.abs(u1.astype(np.float64) - float(cd))
    if Dl > 0:
        margin = np.minimum(margin, np.abs(u1.astype(np.float64) - float(edge)))
    return s, margin


# ---- the surface at y -----------------------------------------------------------------------------------------------------------------------
def surface_records(V, Fc, mat5, normals, face, bary, w):
    """mesh (V [nV,3], Fc [nT,3], mat5 [nV,5] PERCEPTUAL roughness, normals [nV,3] or None), the hit faces [n], their (u, v) [n,2] and the
    incoming directions w [n,3] (its dtype rules) -> rec [n,32] in the layout of mc_shade_ref.point_setup, decisions.  The rules of
    Relighter.surface: flat normal turned against the ray, supplied normals interpolated and not turned, roughness squared once."""
    dt = w.dtype
    bary = bary.to(dt)
    y = RR.interpolate(V.to(dt), Fc, face, bary)
    m = RR.interpolate(mat5.to(dt), Fc, face, bary)
    m = torch.cat([m[:, 0:1], m[:, 1:2] * m[:, 1:2], m[:, 2:5]], -1)
    one = torch.ones(len(face), dtype=F64)
    if normals is None:
        corner = V.to(dt)[Fc.long()[face.long()]]
        g = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
        side = (g * w).sum(-1, keepdim=True)
        flip = (side[:, 0] > 0, (side[:, 0].abs() / torch.clamp(torch.norm(g, dim=-1), min=1e-30)).double())
        g = torch.where(side > 0, -g, g)
    else:
        g = RR.interpolate(normals.to(dt), Fc, face, bary)
        flip = (one > 0, one)
    rec, dec = R.point_setup(y, -w, F.normalize(g, dim=-1), m, None, None)
    return rec, {'flip': flip, 'ortho_n2': (dec['ortho_n'][0], dec['ortho_n'][1].double()), 'ortho_r2': (dec['ortho_r'][0], dec['ortho_r'][1].double())}


# ---- the secondary sample -------------------------------------------------------------------------------------------------------------------
def cosine_dir(rec, az_t, el):
    """mc_shade_ref.diffuse_dirs for one (azimuth, elevation) PER ROW, no rotation: rec [n,32], az_t, el [n] -> [n,3]"""
    TWO_PI = ER._pi(rec.dtype)[1]
    az = az_t * TWO_PI
    es, cz = torch.sqrt(el + 1e-7), torch.sqrt(1 - el + 1e-7)
    cx, cy = (es * torch.cos(az))[:, None], (es * torch.sin(az))[:, None]
    return cx * rec[:, 15:18] + cy * rec[:, 18:21] + cz[:, None] * rec[:, 3:6]


def ggx_dir(rec, az_t, el):
    """mc_shade_ref.specular_dirs for one (azimuth, elevation) PER ROW, no rotation"""
    TWO_PI = ER._pi(rec.dtype)[1]
    a = rec[:, 10]
    cost = torch.sqrt((1.0 - el + 1e-6) / (1.0 + (a * a - 1.0) * el + 1e-6) + 1e-6)
    sint = torch.sqrt(1 - cost * cost + 1e-6)
    phi = TWO_PI * az_t
    return (torch.cos(phi) * sint)[:, None] * rec[:, 21:24] + (torch.sin(phi) * sint)[:, None] * rec[:, 24:27] + cost[:, None] * rec[:, 6:9]


def secondary(rec, strat, u2, u3, table, geometry_type, cell=None):
    """rec [n,32], strat [n] int64 numpy, u2, u3 [n] float32 numpy, table = (cdf numpy int64, gh, gw) or None; cell [n] numpy: the cells to
    read p_l from in the place of the restated ones (a discrete fact the GPU tier takes from the device, as tests/test_relight_mis_gpu.py
    does) -> w2, o2 [n,3], dead2 [n] bool, p_l [n] (0 without a table), decisions {'dead2', 'cell2'}"""
    dt = rec.dtype
    n = rec.shape[0]
    t2, t3 = torch.from_numpy(np.ascontiguousarray(u2)).to(dt), torch.from_numpy(np.ascontiguousarray(u3)).to(dt)
    st = torch.from_numpy(np.ascontiguousarray(strat))
    w2 = torch.where((st == 0)[:, None], cosine_dir(rec, t2, t3), ggx_dir(rec, t2, t3))
    pl = torch.zeros(n, dtype=dt)
    cell_margin = torch.ones(n, dtype=F64)
    if table is not None:
        cdf, gh, gw = table
        row, col, x1, x2, _ = ER.draw(cdf, gh, gw, u2, u3)
        as_t = lambda z: torch.from_numpy(np.ascontiguousarray(z))
        x1, x2 = as_t(x1).to(dt), as_t(x2).to(dt)                   # (float32: the kernel rounds the float64 residuals to float)
        u = (as_t(col).to(dt) + x2) / torch.tensor(float(gw), dtype=dt)
        v = 1.0 - (as_t(row).to(dt) + x1) / torch.tensor(float(gh), dtype=dt)
        wl, _ = ER.grid_dir(u, v)
        light = st == 2
        w2 = torch.where(light[:, None], wl, w2)
        cell_b, v_b, margin_b = ER.lookup_cell(w2, gh, gw)
        if cell is None:
            cell = np.where(light.numpy(), row * gw + col, cell_b)
        else:
            margin_b = torch.ones_like(margin_b)                       # given, not decided here
        pl = ER.pdf_light(cdf, gh, gw, cell, torch.where(light, v, v_b))
        cell_margin = torch.where(light, cell_margin, margin_b.double())
    o2 = rec[:, 29:32] + w2 * 1e-5
    nw = (rec[:, 3:6] * w2).sum(-1)
    dead2 = (st >= 1) & (nw < -1e-6) & (geometry_type == 0)
    dmargin = torch.where((st >= 1) & torch.tensor(geometry_type == 0), (nw + 1e-6).abs().double(), torch.ones(n, dtype=F64))
    return w2, o2, dead2, pl, {'dead2': (nw < -1e-6, dmargin), 'cell2': (cell_margin > 0, cell_margin)}


def radiance(rec, w2, pl, Le, Dd, Ds, Dl, geometry_type, clamp=0.0):
    """L_o of ONE sample w2 that fetched Le: the per-sample term of envsample_ref.mis_estimator, not averaged (test_relight_bounce_cpu checks
    it IS D times mis_estimator of a one-sample set) -> L_o (capped per channel when clamp > 0), its diffuse part, its specular part [n,3]"""
    D = Dd + Ds + Dl
    PI = ER._pi(rec.dtype)[0]
    nol, nov, dg, G, fc, pcode, pact = ER.brdf_terms(rec, w2[:, None], geometry_type)
    pd = nol / PI
    pmix = ((Dd * pd + Ds * pact) + Dl * pl[:, None]) / D
    dterm = torch.where((nol > 0) & (pmix > 0), pd / torch.where(pmix > 0, pmix, torch.ones_like(pmix)), torch.zeros_like(pd))
    S = 1.0 + pact / (pcode + 1e-5)
    W = S * dg * G / (4 * nov * pmix + 1e-5)
    m, alb = rec[:, 9:10], rec[:, 11:14]
    F0 = 0.04 * (1 - m) + m * alb
    Fr = F0 + (1.0 - F0) * fc
    spec = Fr * Le * W
    diff = alb * (1 - m) * Le * dterm
    Lo = diff + spec
    if clamp > 0:
        Lo = torch.clamp(Lo, max=clamp)
    return Lo, diff, spec


# ---- the estimator with one bounce ------------------------------------------------------------------------------------------------------------
def _primary(pt, w, L, pdf_l, Dd, Ds, Dl, geometry_type):
    """-> diffuse_lin, spec_lin [P,3] of the primary estimator (two-strategy when Dl == 0) for the radiance L [P D,3]"""
    P_, D = pt.shape[0], Dd + Ds + Dl
    if Dl == 0:
        rgb, _, _, spec, _ = R.estimator(pt, pt[:, None, 9:14], w.reshape(P_, D, 3), L.reshape(P_, D, 3), Dd, Ds, geometry_type)
        return rgb - spec, spec
    _, diff, spec = ER.mis_estimator(pt, w.reshape(P_, D, 3), L.reshape(P_, D, 3), pdf_l.reshape(P_, D), Dd, Ds, Dl, geometry_type)
    return diff, spec


def bounce(pt, w, pdf_l, state, face, bary, blocked2, key, mesh, env, convention, rot, clamp, Dd, Ds, Dl, geometry_type, table=None, strat=None, cell2=None):
    """pt [P,32], w [P D,3] the primary directions and pdf_l [P D] their p_l (None without a table), in the dtype to evaluate in; state [P D]
    (int tensor), face [P D], bary [P D,2], blocked2 [P D] bool: the discrete facts; key [P] integers or None; mesh = (V, Fc, mat5 perceptual,
    normals | None); table = (cdf, gh, gw) for Dl > 0; strat [P D] overrides the restated choice, cell2 [P D] the restated cells of the
    secondary directions.
    -> dict: rgb, diffuse, spec, indirect [P,3], indirect_sd / indirect_ss (the parts of `indirect` that come from the secondary's diffuse /
    specular term, uncapped, each as the pair (through the primary's diffuse term, through its specular term)), sec_o, sec_d [P D,3], pdf_l2 [P D], strategy [P D] numpy (-1 where not bounced), dec"""
    dt = pt.dtype
    P_, D = pt.shape[0], Dd + Ds + Dl
    V, Fc, mat5, normals = mesh
    state = torch.as_tensor(state).long().reshape(-1)
    u1, u2, u3 = variates(np.zeros(P_, np.int64) if key is None else np.asarray(key), D)
    s_all, s_margin = strategy(u1, Dd, Ds, Dl)
    sec = (state == BOUNCED) | (state == BOUNCED_DEAD)
    idx = torch.nonzero(sec)[:, 0]
    s_row = s_all.reshape(-1)[idx.numpy()] if strat is None else np.asarray(strat).reshape(-1)[idx.numpy()].astype(np.int64)
    rec, dec_s = surface_records(V, Fc, mat5, normals, torch.as_tensor(face).reshape(-1)[idx], torch.as_tensor(bary).reshape(-1, 2)[idx], w[idx])
    w2, o2, dead2, pl2, dec_2 = secondary(rec, s_row, u2.reshape(-1)[idx.numpy()], u3.reshape(-1)[idx.numpy()], table if Dl > 0 else None,
                                          geometry_type, None if cell2 is None else np.asarray(cell2).reshape(-1)[idx.numpy()].astype(np.int64))
    Le, _ = RR.env_lookup(env, w2, convention, rot, clamp)
    Lo, Lo_d, Lo_s = radiance(rec, w2, pl2, Le, Dd, Ds, Dl, geometry_type, clamp)
    lit2 = (state[idx] == BOUNCED) & ~torch.as_tensor(blocked2).reshape(-1)[idx].bool()
    Ld, dec = RR.env_lookup(env, w, convention, rot, clamp)
    Ld = torch.where((state == FREE)[:, None], Ld, torch.zeros_like(Ld))
    zero = torch.zeros(P_ * D, 3, dtype=dt)
    put = lambda x: zero.index_copy(0, idx, torch.where(lit2[:, None], x, torch.zeros_like(x)))
    pl = torch.zeros(P_ * D, dtype=dt) if pdf_l is None else pdf_l
    dif, spec = _primary(pt, w, Ld, pl, Dd, Ds, Dl, geometry_type)
    ind = sum(_primary(pt, w, put(Lo), pl, Dd, Ds, Dl, geometry_type))
    ind_sd = _primary(pt, w, put(Lo_d), pl, Dd, Ds, Dl, geometry_type)
    ind_ss = _primary(pt, w, put(Lo_s), pl, Dd, Ds, Dl, geometry_type)
    full = lambda x, fill: torch.full((P_ * D,) + tuple(x.shape[1:]), fill, dtype=x.dtype).index_copy(0, idx, x)
    dec = {k: (s.reshape(P_, D), m.reshape(P_, D)) for k, (s, m) in dec.items()}
    for k, (s, m) in {**dec_s, **dec_2}.items():                       # lanes that do not bounce decide nothing: margin 1
        dec[k] = (full(s, True).reshape(P_, D), full(m.double(), 1.0).reshape(P_, D))
    sm = torch.where(sec, torch.from_numpy(s_margin.reshape(-1)), torch.ones(P_ * D, dtype=F64))
    dec['strategy'] = (sm > 0, sm.reshape(P_, D))
    strategy_out = np.full(P_ * D, -1, np.int64)
    strategy_out[idx.numpy()] = s_row
    return {'rgb': (dif + spec) + ind, 'diffuse': dif, 'spec': spec, 'indirect': ind, 'indirect_sd': ind_sd, 'indirect_ss': ind_ss,
            'sec_o': full(o2, 0.0), 'sec_d': full(w2, 0.0), 'pdf_l2': full(pl2, 0.0), 'strategy': strategy_out,
            'dead2': full(dead2, False), 'dec': dec}


# ---- brute-force facts (CPU tier) -------------------------------------------------------------------------------------------------------------
def facts(pt, w, o, dead, pdf_l, key, mesh, Dd, Ds, Dl, geometry_type, table=None):
    """everything a lane decides, by brute force in the dtype of pt: the primary closest hit, the secondary direction from it, the second
    shadow ray -> state, face, bary, blocked2 (tensors [P D]), decisions {'hit', 'shadow2'} [P, D]"""
    P_, D = pt.shape[0], Dd + Ds + Dl
    V, Fc, mat5, normals = mesh
    dt = pt.dtype
    _, face, bary, margin = RR.closest_hit(V.to(dt), Fc, o, w)
    dead = torch.as_tensor(dead).bool()
    state = torch.where(dead, torch.full_like(face, DEAD), torch.where(face >= 0, torch.full_like(face, BOUNCED), torch.full_like(face, FREE)))
    face = torch.where(dead, torch.full_like(face, -1), face)
    never = torch.zeros(P_ * D, dtype=torch.bool)
    first = bounce(pt, w, pdf_l, state, face, bary, never, key, mesh, torch.ones(2, 4, 3), 2, None, 0.0, Dd, Ds, Dl, geometry_type, table)
    state = torch.where((state == BOUNCED) & first['dead2'], torch.full_like(state, BOUNCED_DEAD), state)
    idx = torch.nonzero(state == BOUNCED)[:, 0]
    one = torch.ones(P_ * D, dtype=F64)
    blocked2, sh_m = never, one
    if len(idx):
        b2, dec2 = RR.occluded(V.to(dt), Fc, first['sec_o'][idx], first['sec_d'][idx])
        blocked2, sh_m = never.index_copy(0, idx, b2), one.index_copy(0, idx, dec2['shadow'][1].double())
    hit_m = torch.where(dead, one, margin.double())
    return state, face, bary, blocked2, {'hit': ((face >= 0).reshape(P_, D), hit_m.reshape(P_, D)), 'shadow2': (blocked2.reshape(P_, D), sh_m.reshape(P_, D))}


def exempt(dec, keys=EXEMPT_KEYS):
    """[P] bool: points with a discontinuous decision nearer than relight_ref.MARGIN (relight_ref.exempt over this file's keys too)"""
    return RR.exempt(dec, keys)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def corner_scene():
    """three mutually perpendicular unit quads meeting at the origin, six triangles wound so that their flat normals point into the
    octant they enclose, the whole turned by relight_ref.ROT so that no normal lies on an axis (no tie in a frame's choice)
    -> V [7,3] float32, Fc [6,3] int64, the three inward unit normals [3,3] float64"""
    V = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=F64)
    Fc = torch.tensor([[0, 1, 4], [0, 4, 2], [0, 2, 5], [0, 5, 3], [0, 3, 6], [0, 6, 1]], dtype=torch.long)      # z = 0, x = 0, y = 0
    Rm = torch.as_tensor(np.asarray(RR.ROT, np.float64))
    nrm = torch.eye(3, dtype=F64)[[2, 0, 1]] @ Rm.T
    return (V @ Rm.T).float(), Fc, nrm


def corner_points(P_, seed=0):
    """P points on the three faces of corner_scene in turn (inside the unit quads, away from the edges), normals = the faces', views in the
    enclosed octant, random materials -> dict(pts, view, normals, mat5 with ALPHA (estimator_materials applied), rand_d, rand_s, cls)"""
    g = torch.Generator().manual_seed(4100 + seed + 17 * P_)
    V, Fc, nrm = corner_scene()
    Rm = torch.as_tensor(np.asarray(RR.ROT, np.float64))
    k = torch.arange(P_) % 3                                            # the face: z = 0, x = 0, y = 0
    ab = 0.08 + 0.5 * torch.rand(P_, 2, generator=g, dtype=F64)
    local = torch.zeros(P_, 3, dtype=F64)
    axes = torch.tensor([[0, 1], [1, 2], [2, 0]])[k]                    # the two in-plane axes of each face
    local.scatter_(1, axes, ab)
    view = 0.15 + torch.rand(P_, 3, generator=g, dtype=F64)
    mat5 = torch.cat([torch.rand(P_, 1, generator=g), 0.3 + 0.6 * torch.rand(P_, 1, generator=g), 0.1 + 0.8 * torch.rand(P_, 3, generator=g)], -1)
    mat5[:, 1] = mat5[:, 1] ** 2
    return {'pts': (local @ Rm.T).float(), 'view': (F.normalize(view, dim=-1) @ Rm.T).float(), 'normals': nrm[k].float(), 'mat5': mat5.float(),
            'rand_d': torch.rand(P_, generator=g), 'rand_s': torch.rand(P_, generator=g), 'cls': torch.zeros(P_, dtype=torch.long)}


def vertex_materials(nV, seed=0):
    """[nV,5] metallic, PERCEPTUAL roughness in [0.3, 0.9], albedo in [0.1, 0.9]"""
    g = torch.Generator().manual_seed(5200 + seed)
    return torch.cat([torch.rand(nV, 1, generator=g), 0.3 + 0.6 * torch.rand(nV, 1, generator=g), 0.1 + 0.8 * torch.rand(nV, 3, generator=g)], -1)


def primary_rays(pt, tab_d, tab_s, tab_l, rand_l, table, geometry_type):
    """the primary sample set in the dtype of pt -> w, o [P D,3], dead [P D] bool, pdf_l [P D] or None (two-strategy: tab_l None)"""
    Dd, Ds = tab_d.shape[0], tab_s.shape[0]
    if tab_l is None:
        w, o = R.dirs(pt, tab_d.to(pt.dtype), tab_s.to(pt.dtype))
        dead, _ = R.dead_rays(pt, w, Dd, Ds, geometry_type)
        return w, o, dead, None
    cdf, gh, gw = table
    w, o, dead, _, pdf, _, _ = ER.mis_rays(pt, tab_d, tab_s, tab_l, rand_l, cdf, gh, gw, geometry_type)
    return w, o, dead, pdf


# ---- the committed cases of the GPU tier (checked on the CPU by tests/test_relight_bounce_cpu.py) ------------------------------------------------
SHAPES = ((1, 1, 0), (3, 2, 0), (32, 32, 0), (33, 32, 0), (96, 160, 0), (16, 16, 32), (33, 32, 7))     # Dl = 0: the two-strategy primary
PS = (1, 65, 1000)
MESHES = ('sphere', 'corner')            # relight_ref.scene(3): the sphere under a quad; corner_scene()


def cases():
    """(index, P, Dd, Ds, Dl, mesh, geometry type): every P x shape on both meshes, one mesh under each geometry type, in turn"""
    out = []
    for P_ in PS:
        for Dd, Ds, Dl in SHAPES:
            for k, mesh in enumerate(MESHES):
                out.append((len(out), P_, Dd, Ds, Dl, mesh, (len(out) // 2 + k) % 2))
    return out


def case_inputs(i, P_, Dd, Ds, Dl, mesh):
    """-> dict: c (point candidates: pts, view, normals, mat5 with alpha, rand_d, rand_s, rand_l, cls), tab_d, tab_s, tab_l (None for Dl = 0),
    V, Fc, vmat5 (per vertex, perceptual roughness), normals, key [P] numpy int64 in [0, 2^32), env, conv, rot, clamp (envsample_ref.
    env_of_case).  The sphere carries vertex normals (its own radial ones, the quad's pointing down at it): the facets of an icosphere come
    in mirror pairs whose flat normals tie the frame's choice (|n.y| = |n.z| up to rounding) -- a coin toss in float32 that no seed
    avoids -- while an interpolated normal ties on a curve only; the corner has flat normals, turned out of the axes."""
    normals = None
    if mesh == 'sphere':
        c, tab_d, tab_s, _ = ER.candidates(P_, Dd, Ds, max(Dl, 1))
        V, Fc = RR.scene(3)
        normals = torch.cat([F.normalize(V[:-4], dim=-1), torch.tensor([[0.0, 0.0, -1.0]]).expand(4, 3)]).contiguous()
    else:
        c = corner_points(P_, seed=i)
        c['rand_l'] = torch.rand(P_, 2, generator=torch.Generator().manual_seed(77 + i))
        tab_d, tab_s = RR.sample_table(Dd), RR.sample_table(Ds)
        V, Fc, _ = corner_scene()
    env, conv, rot, clamp = ER.env_of_case(i)
    key = (np.arange(P_, dtype=np.int64) * 2654435761 + 40503 * (i + 1)) & 0xffffffff
    return {'c': c, 'tab_d': tab_d, 'tab_s': tab_s, 'tab_l': RR.sample_table(Dl) if Dl else None, 'V': V, 'Fc': Fc,
            'vmat5': vertex_materials(len(V), i), 'normals': normals, 'key': key, 'env': env, 'conv': conv, 'rot': rot, 'clamp': clamp}
