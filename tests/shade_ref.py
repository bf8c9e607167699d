"""Plain torch restatement of the Stage-I shading and compositing kernels (nero_amd/csrc/shade.hip, the Jacobian kernels of encode.hip):
one function per operation, over the arrays the kernels take, written with differentiable torch ops only and dtype-generic (one source
serves float64 and float32).  Backward references are torch.autograd of these forwards (`vjp` below), so every tie rule is torch's own:
`clamp` passes the gradient on its bounds, `relu` does not at 0.  Pieces oracle/nero_oracle.py already states are called, not restated.
Each forward also returns the DECISIONS it took: name -> (side [bool per row / element], distance to the boundary); the tests use them
for branch coverage and for the margins of derived boundaries (tests/test_shade_ref_cpu.py, tests/test_shade_kernels_gpu.py)."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import nero_oracle as O

EPS32 = 2.0 ** -24
# the shapes of the GPU tier (n, R, T): every n across the 128-thread blocks, the 64-row blocks and the 64-row pad; T = 1 / 5 / 160 so that
# idx[k] // T picks different rays and poses inside one block
PER_SAMPLE = [(1, 3, 1), (63, 3, 160), (64, 4, 5), (65, 5, 5), (127, 6, 160), (128, 7, 1), (129, 5, 160), (200, 7, 5)]
COMPOSITE_WAVE_T, COMPOSITE_THREAD_T = (1, 2, 63, 64, 65, 128, 129, 192), (193, 200)      # <= 192: one wavefront per ray (64-lane chunks)
WAVE_R, THREAD_R = (1, 3, 4, 5, 67), (1, 63, 65, 130)                                      # 4 resp. 64 rays per workgroup


def row_pad(n):
    return (n + 63) // 64 * 64


def ray_of(idx, T):
    return torch.div(idx.long(), T, rounding_mode='floor')


def vjp(outs, cots, leaves):
    """sum <cot, out> back to the leaves (unused leaf -> zeros); cots may hold None"""
    loss = sum((o * c).sum() for o, c in zip(outs, cots) if c is not None)
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, gs)]


def leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


# ---- NeuS alpha, shading frame, eikonal term (compute_sdf_alpha / render_core) ----------------------------------------------------------
def sdf_alpha(sdf, grad, dist, d, ray, inv_s, anneal):
    """sdf [n], grad [n,3], dist [n], d [R,3] (unnormalised), ray [n] long, inv_s [n] (= clamp(exp(10 variance), 1e-6, 1e6) per row, so that
    its per-row gradient is the kernel's dinv) -> alpha [n], geo [n,8] = {nhat, NoV, refl, |grad|}, gerr [n], decisions"""
    dh = F.normalize(d, dim=-1)[ray]
    tc = (dh * grad).sum(-1)
    ic = -(F.relu(-tc * 0.5 + 0.5) * (1.0 - anneal) + F.relu(-tc) * anneal)
    en, ep = sdf + ic * dist * 0.5, sdf - ic * dist * 0.5
    pc, nc = torch.sigmoid(ep * inv_s), torch.sigmoid(en * inv_s)
    raw = (pc - nc + 1e-5) / (pc + 1e-5)
    alpha = raw.clamp(0.0, 1.0)
    n = F.normalize(grad, dim=-1)
    v = -dh
    nov = (n * v).sum(-1, keepdim=True)
    refl = nov * n * 2 - v
    gn = torch.linalg.norm(grad, dim=-1)
    geo = torch.cat([n, nov, refl, gn[:, None]], -1)
    dec = {'relu_half': (-tc * 0.5 + 0.5 > 0, (-tc * 0.5 + 0.5).abs()), 'relu_cos': (-tc > 0, tc.abs()),
           'raw_lo': (raw >= 0, raw.abs()), 'raw_hi': (raw <= 1, (raw - 1).abs()), 'grad_zero': (gn >= 1e-12, gn)}
    return alpha, geo, (gn - 1.0) ** 2, dec


def inv_s_of(variance, dtype):
    return torch.exp(variance.to(dtype) * 10.0).clamp(1e-6, 1e6)


def sdf_alpha_bwd(sdf, grad, dist, d, ray, inv_s, anneal, d_alpha, d_gerr, d_geo, dtype=torch.float64):
    """-> d_sdf [n], d_grad [n,3], dinv [n]; d_gerr / d_geo [n,8] (column 7 carries nothing) may be None"""
    c = lambda t: None if t is None else t.to(dtype)
    ls = [leaf(sdf, dtype), leaf(grad, dtype), leaf(inv_s.to(dtype).expand(sdf.shape[0]), dtype)]
    alpha, geo, gerr, _ = sdf_alpha(ls[0], ls[1], c(dist), c(d), ray, ls[2], anneal)
    return vjp([alpha, gerr, geo[:, :7]], [c(d_alpha), c(d_gerr), None if d_geo is None else c(d_geo)[:, :7]], ls)


def sdf_alpha_term_sizes(sdf, grad, dist, d, ray, inv_s, anneal, d_alpha):
    """float64 sizes of the terms whose DIFFERENCE the alpha gradients are, per row: alpha = (pc - nc + 1e-5) / (pc + 1e-5) pulls on the
    previous and the next cdf with opposite signs, each pull of size |d_alpha| sigmoid'(.) inv_s / (pc + 1e-5).  d_sdf is their sum, dinv
    the same weighted by e_prev / e_next, the ray-cosine part of d_grad by dist / 2.  On a sample with no section (dist == 0), a grazing or
    a saturated one (alpha == 1 exactly) the pulls cancel to 1e-5 ... 1e-30 of their size: float32 -- and, at 1e-16, float64 -- cannot
    resolve such a row relative to ITSELF, in any implementation, so the GPU tier measures a row of these three outputs against the larger of
    its own magnitude and this size.  -> (T_sdf [n], T_grad [n], T_dinv [n])"""
    sdf, grad, dist, d, inv_s, d_alpha = [t.double() for t in (sdf, grad, dist, d, inv_s, d_alpha)]
    dh = F.normalize(d, dim=-1)[ray]
    tc = (dh * grad).sum(-1)
    ic = -(F.relu(-tc * 0.5 + 0.5) * (1.0 - anneal) + F.relu(-tc) * anneal)
    en, ep = sdf + ic * dist * 0.5, sdf - ic * dist * 0.5
    pc, nc = torch.sigmoid(ep * inv_s), torch.sigmoid(en * inv_s)
    pull = d_alpha.abs() * (pc * (1 - pc) + nc * (1 - nc)) / (pc + 1e-5)
    return pull * inv_s, pull * inv_s * dist.abs() * 0.5, pull * torch.maximum(ep.abs(), en.abs())


# ---- light-MLP input encodings ----------------------------------------------------------------------------------------------------------
def sphere_dir(p, v):
    q = O.offset_points_to_sphere(p)
    return F.normalize(q + v * O.sphere_exit_dist(q, v), dim=-1)


def materials(m_raw, r_raw, a_raw):
    """raw heads [n,4] -> mat [n,8] = {metallic, roughness, albedo(3), 0, 0, 0}"""
    z = torch.zeros_like(a_raw[:, :3])
    return torch.cat([torch.sigmoid(m_raw[:, :1]), torch.sigmoid(r_raw[:, :1]), torch.sigmoid(a_raw[:, :3]), z], -1)


def shade_encode(p, nh, refl, rough, sphere):
    """p, nh, refl [n,3], rough [n,1] -> Xd, Xs [n,72|144], Xi [n,128], Xo [n,96], decisions"""
    enc_r = O.ide(refl, rough)
    Xd, Xs = O.ide(nh, 1.0), enc_r
    dec = {}
    if sphere:
        Xd = torch.cat([Xd, O.ide(sphere_dir(p, nh), 1.0)], -1)
        Xs = torch.cat([Xs, O.ide(sphere_dir(p, refl), rough)], -1)
        pn = torch.linalg.norm(p, dim=-1)
        dec['sphere_pull'] = (pn > 0.999, (pn - 0.999).abs())
    pe = O.pos_enc(p, 8)
    z = torch.zeros_like(p[:, :1])
    Xi = torch.cat([pe, enc_r, z.expand(-1, 5)], -1)
    Xo = torch.cat([pe, O.pos_enc(refl, 6), z.expand(-1, 6)], -1)
    return Xd, Xs, Xi, Xo, dec


def shade_encode_bwd(p, geo, mat, dXd, dXs, dXi, dmat, extra, sphere, dtype=torch.float64):
    """the kernel's inputs (mat AFTER the sigmoid: the raw heads are its logit, so that autograd supplies m (1 - m)) ->
    d_geo [n,8] = {d_nhat, dmat[5], d_refl, 0}, dm_raw [n], dr_raw [n], da_raw [n,3]"""
    c = lambda t: None if t is None else t.to(dtype)
    nh, refl = leaf(geo[:, 0:3], dtype), leaf(geo[:, 4:7], dtype)
    raws = [leaf(torch.logit(mat[:, i:j].to(torch.float64)), dtype) for i, j in ((0, 1), (1, 2), (2, 5))]
    m, r, a = [torch.sigmoid(t) for t in raws]
    if dtype == torch.float64:                 # the kernel reads mat itself: sigmoid(logit(x)) is x to one rounding, m (1 - m) likewise
        assert float((torch.cat([m, r, a], -1).detach() - mat[:, :5].double()).abs().max()) < 1e-14
    Xd, Xs, Xi, _, _ = shade_encode(c(p), nh, refl, r, sphere)
    dm = c(dmat)
    outs, cots = [Xd, Xs, Xi[:, 51:123], m, r, a], [c(dXd), c(dXs), c(dXi)[:, 51:123], dm[:, 0:1], dm[:, 1:2], dm[:, 2:5]]
    if extra is not None:
        outs, cots = outs + [refl, r], cots + [c(extra)[:, :3], c(extra)[:, 3:4]]
    g = vjp(outs, cots, [nh, refl] + raws)
    d_geo = torch.cat([g[0], dm[:, 5:6], g[1], torch.zeros_like(dm[:, :1])], -1)
    return d_geo, g[2][:, 0], g[3][:, 0], g[4]


# ---- human ("photo capturer") light input --------------------------------------------------------------------------------------------
def human_encode(p, refl, rough, poses):
    """p, refl [n,3], rough [n,1], poses [n,3,4] (per SAMPLE: poses_per_ray[idx // T]) -> Xh [n,24], hmask [n], decisions"""
    inter, dists, hits0 = O.camera_plane_intersection(p, refl, poses)
    mean = inter[..., :2] * 0.3
    var = rough * (dists[:, None] * 0.3) ** 2
    rad = torch.norm(mean, dim=-1)
    hits = (hits0 & (rad < 1.5) & (dists > 0)).to(p.dtype).unsqueeze(-1)
    mean, var = mean * hits, (var * hits).expand(mean.shape[0], 2)
    dz = (poses[:, :, :3] @ refl[:, :, None])[:, 2, 0]
    dec = {'dz_small': (dz.abs() > 1e-4, (dz.abs() - 1e-4).abs()), 'dist_pos': (dists > 0, dists.abs()),
           'radius': (rad < 1.5, (rad - 1.5).abs()), 'hit': (hits[:, 0] > 0, torch.ones_like(rad))}
    return O.ipe(mean, var, 0, 6), hits[:, 0], dec


def human_encode_bwd(p, geo, mat, poses, dXh, dtype=torch.float64):
    """-> extra [n,4] = {d_refl(3), d_rough}"""
    refl, rough = leaf(geo[:, 4:7], dtype), leaf(mat[:, 1:2], dtype)
    Xh, _, _ = human_encode(p.to(dtype), refl, rough, poses.to(dtype))
    g = vjp([Xh], [dXh.to(dtype)], [refl, rough])
    return torch.cat(g, -1)


# ---- split-sum combine -----------------------------------------------------------------------------------------------------------------
def _combine_parts(nov, mat, Ld, Ls, Li, Lo, lut, exp_max, Lh, hmask):
    """nov [n], mat [n,>=5], raw heads [n,4], lut [1,256,256,2]; Lh [n,4] / hmask [n] or None -> dict of every intermediate of
    AppShadingNetwork.forward, and the decisions"""
    act = O._exp_act(exp_max)
    m, r, a = mat[:, 0:1], mat[:, 1:2], mat[:, 2:5]
    dl, direct, indirect = act(Ld[:, :3]), act(Ls[:, :3]), act(Li[:, :3])
    dec = {f'exp_max_{k}': (t[:, :3] <= exp_max, (t[:, :3] - exp_max).abs()) for k, t in (('d', Ld), ('s', Ls), ('i', Li))}
    hl, hw = 0, 0
    if Lh is not None:
        h = O._exp_act(0.0)(Lh) * hmask[:, None]
        hl, hw_raw = h[:, :3], h[:, 3:]
        hw = torch.clamp(hw_raw, 0.0, 1.0)
        dec.update(h_raw=(Lh <= 0, Lh.abs()), hmask=(hmask > 0, torch.ones_like(hmask)), hw_hi=(hw_raw[:, 0] <= 1, (hw_raw[:, 0] - 1).abs()),
                   hw_lo=(hw_raw[:, 0] >= 0, hw_raw[:, 0].abs()))
    occ = Lo[:, :1] * 0.5 + 0.5
    oc = torch.clamp(occ, 0.0, 1.0)
    sl = indirect * oc + (hl * hw + direct * (1 - hw)) * (1 - oc)
    u, v = torch.clamp(nov, 0.0, 1.0), torch.clamp(r[:, 0], 0.0, 1.0)
    fg = O.fg_lut_fetch(lut.to(nov.dtype), u, v)
    da, sa = (1 - m) * a, 0.04 * (1 - m) + m * a
    sref = sa * fg[:, 0:1] + fg[:, 1:2]
    lin = da * dl + sref * sl
    srgb = O.linear_to_srgb(lin)
    uu, vv = u * 256 - 0.5, v * 256 - 0.5
    tex = lambda t: torch.minimum(t - torch.floor(t), torch.ceil(t) - t)          # distance to a texel edge (0 at integers)
    dec.update(occ_lo=(occ[:, 0] >= 0, occ[:, 0].abs()), occ_hi=(occ[:, 0] <= 1, (occ[:, 0] - 1).abs()),
               knee=(lin <= 0.0031308, (lin - 0.0031308).abs()), out_hi=(srgb <= 1, (srgb - 1).abs()), out_lo=(srgb >= 0, srgb.abs()),
               nov_lo=(nov >= 0, nov.abs()), nov_hi=(nov <= 1, (nov - 1).abs()), r_lo=(r[:, 0] >= 0, r[:, 0].abs()),
               r_hi=(r[:, 0] <= 1, (r[:, 0] - 1).abs()),
               u_first=(uu >= 0, uu.abs()), u_last=(uu <= 255, (uu - 255).abs()), v_first=(vv >= 0, vv.abs()), v_last=(vv <= 255, (vv - 255).abs()),
               u_texel=(torch.ones_like(uu, dtype=torch.bool), torch.where((uu > 0) & (uu < 255), tex(uu), torch.ones_like(uu))),
               v_texel=(torch.ones_like(vv, dtype=torch.bool), torch.where((vv > 0) & (vv < 255), tex(vv), torch.ones_like(vv))))
    return dict(m=m, r=r, a=a, dl=dl, direct=direct, indirect=indirect, hl=hl, hw=hw, occ=occ, oc=oc, sl=sl, da=da, sa=sa, sref=sref, lin=lin,
                color=torch.clamp(srgb, 0.0, 1.0)), dec


def combine_fwd(nov, mat, Ld, Ls, Li, Lo, lut, exp_max, Lh=None, hmask=None):
    """-> color [n,3], occ_prob [n] (unclamped), decisions"""
    q, dec = _combine_parts(nov, mat, Ld, Ls, Li, Lo, lut, exp_max, Lh, hmask)
    return q['color'], q['occ'][:, 0], dec


def inter_results(nov, mat, Ld, Ls, Li, Lo, lut, exp_max, Lh=None, hmask=None):
    """-> rec [n,32] in the layout of nero_shade_inter_results (AppShadingNetwork.forward with inter_results=True)"""
    q, _ = _combine_parts(nov, mat, Ld, Ls, Li, Lo, lut, exp_max, Lh, hmask)
    cs = lambda t: torch.clamp(O.linear_to_srgb(t), 0, 1)
    z = torch.zeros_like(q['lin'])
    hum = O.linear_to_srgb(q['hl'] * q['hw']) if Lh is not None else O.linear_to_srgb(z)
    return torch.cat([q['sa'], torch.clamp(q['sref'], 0, 1), cs(q['sl']), cs(q['sref'] * q['sl']), q['da'], cs(q['dl']), cs(q['da'] * q['dl']),
                      q['m'], q['r'], q['oc'], q['indirect'] * q['oc'], hum, z[:, :2]], -1)


def combine_bwd(nov, mat, Ld, Ls, Li, Lo, lut, exp_max, d_color, d_occ, Lh=None, hmask=None, dtype=torch.float64, want_lut_size=False):
    """-> dLd, dLs, dLi [n,4], dLo [n,4], dmat [n,8] = {d_metallic, d_rough (LUT part), d_albedo(3), d_NoV (LUT part), 0, 0}, dLh [n,4] | None.
    want_lut_size: instead, the size [n] of the terms the two LUT gradients (d_rough, d_NoV) are differences of: they are 256 x (difference
    of neighbouring texels) x the pull on specular_ref, i.e. differences of table values of the size of specular_ref itself scaled by 256 --
    the table is smooth, so the difference is 1e-2 ... 1e-4 of its terms and float32 resolves it to no better than that share"""
    c = lambda t: None if t is None else t.to(dtype)
    ls = [leaf(t, dtype) for t in (nov, mat[:, :5], Ld, Ls, Li, Lo)] + ([leaf(Lh, dtype)] if Lh is not None else [])
    color, occ, _ = combine_fwd(ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], lut, exp_max, ls[6] if Lh is not None else None, c(hmask))
    g = vjp([color, occ], [c(d_color), c(d_occ)], ls)
    z = torch.zeros_like(g[0])
    if want_lut_size:
        q, _ = _combine_parts(ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], lut, exp_max, ls[6] if Lh is not None else None, c(hmask))
        g_sref = torch.autograd.grad((q['color'] * c(d_color)).sum(), q['sref'])[0]
        return 256.0 * (g_sref.abs() * q['sref'].abs()).sum(-1).detach()
    dmat = torch.cat([g[1][:, 0:1], g[1][:, 1:2], g[1][:, 2:5], g[0][:, None], z[:, None], z[:, None]], -1)
    return g[2], g[3], g[4], g[5], dmat, (g[6] if Lh is not None else None)


# ---- NeRF++ head -----------------------------------------------------------------------------------------------------------------------
def nerf_head(sig, rgb, dist):
    """sig [n], rgb [n,3] raw, dist [n] -> alpha [n], color [n,3], decisions"""
    alpha = 1.0 - torch.exp(-F.softplus(sig) * dist)
    color = O.linear_to_srgb(torch.exp(torch.clamp(rgb, max=5.0)))
    return alpha, color, {'softplus': (sig > 20, (sig - 20).abs()), 'rgb5': (rgb <= 5, (rgb - 5).abs()), 'dist0': (dist > 0, dist.abs())}


def nerf_head_bwd(sig, rgb, dist, d_alpha, d_color, dtype=torch.float64):
    ls = [leaf(sig, dtype), leaf(rgb, dtype)]
    alpha, color, _ = nerf_head(ls[0], ls[1], dist.to(dtype))
    return vjp([alpha, color], [d_alpha.to(dtype), d_color.to(dtype)], ls)


# ---- compositing -----------------------------------------------------------------------------------------------------------------------
def scatter(a, c, idx, RT, fill):
    alphaRT, colorRT = torch.full((RT,), fill, dtype=a.dtype), torch.full((RT, 3), fill, dtype=a.dtype)
    alphaRT[idx.long()], colorRT[idx.long()] = a, c
    return alphaRT, colorRT


def composite(alphaRT, colorRT):
    """alphaRT [R,T], colorRT [R,T,3] -> weights [R,T], rgb [R,3], decisions.  The transmittance is render_core's own expression, torch.cumprod
    in the working dtype: oracle.transmittance_weights states the same product but accumulates it in float64 whatever the dtype, which would
    make the float32 evaluation of this reference (the measured floor of the GPU tier) better than float32 arithmetic can be; the CPU tier
    pins the two against each other in float64."""
    one = torch.ones_like(alphaRT[:, :1])
    w = alphaRT * torch.cumprod(torch.cat([one, 1.0 - alphaRT + 1e-7], -1), -1)[:, :-1]
    return w, (colorRT * w[..., None]).sum(1), {'opaque': (alphaRT >= 1, (alphaRT - 1).abs()), 'clear': (alphaRT <= 0, alphaRT.abs())}


def composite_bwd(alphaRT, colorRT, d_rgb, dtype=torch.float64):
    ls = [leaf(alphaRT, dtype), leaf(colorRT, dtype)]
    _, rgb, _ = composite(ls[0], ls[1])
    return vjp([rgb], [d_rgb.to(dtype)], ls)


def composite_bwd_term_sizes(alphaRT, colorRT, d_rgb):
    """float64 size [R,T] of the two terms d_alpha is the difference of: dw_i T_i (the sample's own colour) and S_i / (1 - a_i + 1e-7), the
    colour it hides behind it (S_i = sum_{j>i} dw_j w_j, summed here as |dw_j| w_j); behind an opaque sample both are 1e7 times what
    is left of them"""
    a, c, g = alphaRT.double(), colorRT.double(), d_rgb.double()
    w = composite(a, c)[0]
    f = 1.0 - a + 1e-7
    Tr = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), f], -1), -1)[:, :-1]
    q = (c * g[:, None, :]).sum(-1).abs()
    tail = torch.flip(torch.cumsum(torch.flip(q * w, [1]), 1), [1]) - q * w
    return q * Tr + tail / f


# ---- PE Jacobian products --------------------------------------------------------------------------------------------------------------
def pe_vjp(x, e, n_freq, dtype=torch.float64):
    """x [n,3], e [n, 3 (1 + 2 n_freq)] (= e0 + e1) -> J^T e [n,3]"""
    l = leaf(x, dtype)
    return vjp([O.pos_enc(l, n_freq)], [e.to(dtype)], [l])[0]


def pe_jvp(x, t, n_freq, dtype=torch.float64):
    """x, t [n,3] -> J t [n, 3 (1 + 2 n_freq)]"""
    return torch.autograd.functional.jvp(lambda y: O.pos_enc(y, n_freq), x.to(dtype), t.to(dtype))[1]


# ========================================================================================================================================
# edge input builders (float32, seeded): every set is checked on the CPU (tests/test_shade_ref_cpu.py) before a GPU sees it
# ========================================================================================================================================
# Margins of DERIVED boundaries (quantities the kernel computes, which float32 and float64 could put on different sides), in the units of
# the decision's distance.  Sized from the float32 evaluation of this reference on the CPU: the compared quantities are O(1) (texel
# coordinates O(256)) and their float32 value sits within ~1e-6 (texel coordinates: 256 x 6e-8 = 1.5e-5) of the float64 one, so ten times
# that decides alike in both precisions and on the device; |dz| and the section-scaled quantities are O(1e-4) with errors of O(1e-11).
# tests/test_shade_ref_cpu.py asserts, for every committed input set, that no row is closer than this AND that the float32 evaluation takes
# the float64 decisions; the measured closest approaches are listed there.  Decisions not named here sit on DIRECT inputs (exact ties allowed).
MARGINS = {'relu_half': 1e-3, 'relu_cos': 1e-3, 'raw_lo': 1e-6, 'sphere_pull': 1e-4, 'dz_small': 1e-5, 'dist_pos': 1e-4, 'radius': 1e-4,
           'occ_lo': 1e-4, 'occ_hi': 1e-4, 'knee': 1e-5, 'out_hi': 1e-4, 'u_texel': 2e-4, 'v_texel': 2e-4}
# Measured closest approaches over all committed input sets (tests/test_shade_ref_cpu.py asserts them against the table): relu_half 1.0e-2,
# relu_cos 2.9e-2, raw_lo 1.0e-5, sphere_pull 1.1e-3, dz_small 5.0e-5, dist_pos 1.7e-3, radius 5.4e-3, occ_lo 9.3e-4, occ_hi 1.4e-3,
# knee 7.7e-4, out_hi 4.2e-4, u_texel 7.5e-4, v_texel 7.9e-4.
MARGIN = 1e-4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sample_idx(n, RT, g):
    """n flat sample indices in [0, RT), ascending: distinct when they fit, else with repeats (only idx // T is used by the per-sample kernels)"""
    if n <= RT:
        return torch.sort(torch.randperm(RT, generator=g)[:n])[0].int()
    return torch.sort(torch.randint(0, RT, (n,), generator=g))[0].int()


def _keep_clear(x, boundary, margin, push):
    """move entries closer than `margin` to `boundary` away by `push` (deterministic)"""
    near = (x - boundary).abs() < margin
    return torch.where(near, x + push, x)


@functools.lru_cache(maxsize=None)
def alpha_inputs(n, R, T, seed=0):
    """-> dict(sdf4, grad, x4, idx, d, variance); rows 0..: a zero gradient row, |grad| far from 1, both ReLU gates on both sides, raw alpha
    clamped at 0 (needs next-cdf > prev-cdf + 1e-5: only a negative section length does that, iter_cos being <= 0) and one that saturates
    to exactly 1 (raw <= 1 always: the upper clamp is reached only as a tie)"""
    g = _gen(1000 + 7 * n + T + seed)
    d = torch.randn(R, 3, generator=g) * torch.tensor([0.5, 1.0, 3.0])[torch.arange(R) % 3, None]      # unnormalised
    idx = sample_idx(n, R * T, g)
    ray = ray_of(idx, T)
    dh = F.normalize(d, dim=-1)[ray]
    grad = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    # true_cos spread over (-1.2, 1.2) incl. values beyond -1 and +1 (|grad| != 1), away from the gates at 0 and +1
    tc = torch.linspace(-1.9, 1.9, n) if n > 1 else torch.tensor([-0.7])
    tc = _keep_clear(_keep_clear(tc, 0.0, 0.02, 0.05), 1.0, 0.02, 0.05)
    perp = F.normalize(grad - (grad * dh).sum(-1, keepdim=True) * dh, dim=-1)
    grad = dh * tc[:, None] + perp * (0.1 + torch.rand(n, 1, generator=g))       # |grad| from 0.1 to 2.2
    if n > 2:
        grad[2] = 0.0                                                       # zero gradient row (direct input)
    sdf = 0.02 * torch.randn(n, generator=g)
    dist = 0.01 + 0.05 * torch.rand(n, generator=g)
    if n > 4:
        sdf[4], dist[4] = -0.5, 0.5                                         # deep inside, long section: raw saturates towards 1
    if n > 5:
        dist[5] = 0.0                                                       # empty section
    if n > 8:                                                               # a NEGATIVE section (never produced by the sampler, legal for the
        grad[6], sdf[6], dist[6] = -1.5 * dh[6], 0.0, -0.5                  # kernel): next-cdf above prev-cdf, raw alpha below 0 -> clamped, no gradient
    sdf4, x4 = torch.zeros(n, 4), torch.zeros(n, 4)
    sdf4[:, 0], sdf4[:, 1:] = sdf, torch.randn(n, 3, generator=g)
    x4[:, :3], x4[:, 3] = 0.6 * torch.randn(n, 3, generator=g), dist
    return dict(sdf4=sdf4, grad=grad.contiguous(), x4=x4, idx=idx, d=d, variance=torch.tensor([0.45]), ray=ray)


@functools.lru_cache(maxsize=None)
def shading_inputs(n, R, T, seed=0):
    """-> dict for shade_encode / human_encode / combine / inter_results and their backwards.  Direct inputs sit exactly ON their
    boundaries (raw head == exp_max / 0, NoV / roughness / metallic in {0, 1}, hmask in {0, 1}); derived ones on both sides with MARGIN"""
    g = _gen(2000 + 11 * n + T + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    idx = sample_idx(n, R * T, g)
    ray = ray_of(idx, T)
    p = F.normalize(rnd(n, 3), dim=-1) * (0.2 + 0.9 * torch.rand(n, 1, generator=g))      # |p| from 0.2 to 1.1: both sides of 0.999
    pn = torch.linalg.norm(p, dim=-1, keepdim=True)
    p = torch.where((pn - 0.999).abs() < 10 * MARGIN, p * 1.01, p)
    nh = F.normalize(rnd(n, 3), dim=-1)
    v = F.normalize(rnd(n, 3), dim=-1)
    nov = (nh * v).sum(-1, keepdim=True)
    geo = torch.cat([nh, nov, nov * nh * 2 - v, 0.5 + torch.rand(n, 1, generator=g)], -1)
    m_raw, r_raw, a_raw = 2 * rnd(n, 4), 2 * rnd(n, 4), 2 * rnd(n, 4)
    # poses: a rotation about x plus a translation per ray; rays r % 3 == 0 look along the plane (|dz| small on some samples)
    poses = torch.zeros(R, 3, 4)
    for r in range(R):
        a = 0.3 * r
        poses[r, :, :3] = torch.tensor([[1.0, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        poses[r, :, 3] = torch.tensor([0.1 * r, -0.2, 0.5 + 0.4 * (r % 2)])
    # reflection rows with |dz| <= 1e-4 in the human frame: refl inside the plane z = 0 of the ray's pose (+- 5e-5 along its z axis)
    for k in range(3, n, 9):
        zax = poses[ray[k], 2, :3]
        t = F.normalize(torch.linalg.cross(zax, torch.tensor([0.3, 0.5, 0.8])), dim=-1)
        geo[k, 4:7] = t + zax * (5e-5 if k % 2 else -5e-5)
    heads = {k: rnd(n, 4) for k in ('Ld', 'Ls', 'Li')}
    Lo, Lh = 1.5 * rnd(n, 4), 1.5 * rnd(n, 4)                               # occ = 0.5 Lo + 0.5 on both sides of 0 and 1
    Lo[:, 0] = _keep_clear(_keep_clear(Lo[:, 0], -1.0, 4 * MARGIN, 0.01), 1.0, 4 * MARGIN, 0.01)
    if n > 12:                                                              # sigmoids that saturate to exactly 0 / 1 in float32 and float64
        r_raw[5, 0], r_raw[6, 0], m_raw[7, 0], m_raw[8, 0] = -800.0, 40.0, -800.0, 40.0
    mat = materials(m_raw, r_raw, a_raw)
    exp_max = 0.5
    for j, k in enumerate(('Ld', 'Ls', 'Li')):                               # a raw head exactly on exp_max, and far above it
        if n > 8 + j:
            heads[k][6 + j, j] = exp_max
            heads[k][(7 + j) % n, (j + 1) % 3] = exp_max + 2.0
    if n > 12:
        Lh[9, 0], Lh[10, 3], Lh[11, 3] = 0.0, 0.0, 2.0                        # raw human head == 0 and > 0
        geo[5, 3], geo[6, 3], geo[7, 3], geo[8, 3] = 0.0, 1.0, -0.3, 1.0 + 1e-3   # NoV on / beyond both bounds
        mat[5, 1], mat[6, 1], mat[7, 0], mat[8, 0] = 0.0, 1.0, 0.0, 1.0      # roughness / metallic in {0, 1}
        geo[9, 3], mat[9, 1] = 0.5 / 256 - 1e-3, 255.5 / 256 + 1e-3           # first texel (u), last texel (v)
        geo[10, 3], mat[10, 1] = 255.5 / 256 + 1e-3, 0.5 / 256 - 1e-3
        heads['Ld'][11, :] = -9.0                                            # dark rows: lin below the sRGB knee
        heads['Ls'][11, :], heads['Li'][11, :], Lo[11, 0] = -9.0, -9.0, 3.0   # (occ clamps to 1: the bright human light is blended out)
        heads['Ld'][12, :] = 0.5                                             # bright row: sRGB output above 1
        mat[12, 0], mat[12, 2:5] = 0.0, 1.0
    hmask = (torch.arange(n) % 3 != 1).float()                               # stand-alone combine tests: both values
    # rows that land within 3x the margin of a derived boundary of the combine (float64 evaluation, with and without human light) are
    # moved off it: the diffuse head by 0.03 (knee / output clamp), NoV / roughness by 0.18 texel
    from tests.helpers import ref_fg_lut
    lut = ref_fg_lut()
    for _ in range(8):
        moved = False
        for hum in (True, False):
            f = lambda t: t.double()
            dec = combine_fwd(f(geo[:, 3]), f(mat), f(heads['Ld']), f(heads['Ls']), f(heads['Li']), f(Lo), lut, exp_max,
                              f(Lh) if hum else None, f(hmask) if hum else None)[2]
            bad = ((dec['knee'][1] < 3 * MARGINS['knee']) | (dec['out_hi'][1] < 3 * MARGINS['out_hi'])).any(-1)
            heads['Ld'][bad, :3] += 0.03
            bu, bv = dec['u_texel'][1] < 3 * MARGINS['u_texel'], dec['v_texel'][1] < 3 * MARGINS['v_texel']
            geo[bu, 3] += 0.18 / 256
            mat[bv, 1] += 0.18 / 256
            moved = moved or bool(bad.any() or bu.any() or bv.any())
        if not moved:
            break
    assert not moved, 'rows still within 3x the margin of a derived boundary after 8 passes'
    d_color, d_occ = rnd(n, 3), rnd(n)
    return dict(idx=idx, ray=ray, p=p, x4=torch.cat([p, torch.rand(n, 1, generator=g)], -1), geo=geo.contiguous(), m_raw=m_raw, r_raw=r_raw,
                a_raw=a_raw, mat=mat.contiguous(), poses=poses, Lo=Lo, Lh=Lh, hmask=hmask, exp_max=exp_max, d_color=d_color, d_occ=d_occ,
                dXd=rnd(n, 144), dXs=rnd(n, 144), dXi=rnd(n, 128), dXh=rnd(n, 24), extra=rnd(n, 4), dmat=rnd(n, 8), **heads)


@functools.lru_cache(maxsize=None)
def nerf_inputs(n, seed=0):
    g = _gen(3000 + n + seed)
    sig4, rgb4 = 8 * torch.randn(n, 4, generator=g), 3 * torch.randn(n, 4, generator=g)
    dist = 0.02 + torch.rand(n, generator=g)
    if n > 8:
        sig4[1, 0], sig4[2, 0], sig4[3, 0] = 20.0, 20.5, 19.5                 # the softplus switch, on it and on both sides
        rgb4[4, 0], rgb4[5, 1], rgb4[6, 2] = 5.0, 7.0, -12.0                   # rgb raw == 5, above it, and far below (under the sRGB knee)
        dist[7] = 0.0
    return dict(sig4=sig4, rgb4=rgb4, dist=dist, d_alpha=torch.randn(n, generator=g), d_color=torch.randn(n, 3, generator=g))


@functools.lru_cache(maxsize=None)
def composite_inputs(R, T, seed=0):
    """alpha mostly small (a long transmittance tail), with exact 0 and 1 entries; ray 0 (T >= 2) starts with alpha = 1.0 followed by
    0.9999999 (the opaque-sample rows); every third ray holds an opaque sample in its middle"""
    g = _gen(4000 + 13 * R + T + seed)
    a = torch.rand(R, T, generator=g) ** 3 * 0.5
    a[torch.rand(R, T, generator=g) < 0.1] = 0.0
    for r in range(0, R, 3):
        a[r, (T // 2 + r) % T] = 1.0
    a[0, 0] = 1.0
    if T >= 2:
        a[0, 1] = 0.9999999
    if T >= 66:
        a[R - 1, 63], a[R - 1, 64] = 1.0, 1.0                               # opaque on both sides of a 64-lane chunk edge
    c = torch.rand(R, T, 3, generator=g)
    return dict(alpha=a, color=c, d_rgb=torch.randn(R, 3, generator=g))
