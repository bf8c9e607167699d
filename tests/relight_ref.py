"""Plain torch restatement of the relighting kernels (nero_amd/csrc/relight.hip, include/nero_hip_relight.h), dtype-generic: one source serves
float64 and float32.  The per-point record, the directions, the dead rule and the estimator are CALLED from tests/mc_shade_ref.py
(point_setup, dirs, dead_rays, estimator), not restated; this file adds the three environment lookups, "L = 0 where blocked or dead",
barycentric interpolation, the orbit poses and a brute-force closest hit with face ids.

Decisions (`dec`: name -> (side, distance to the boundary)) are carried through as in mc_shade_ref.  The forward value is continuous in
every clamp; what is NOT continuous, and so can be exempted when its margin is under MARGIN, is
  * 'pole': a lookup direction within MARGIN of (but not exactly on) the map's axis, where the azimuth is ill-conditioned -- on a map whose
    first or last row is not constant;
  * 'seam': conventions 0 / 1 on a map whose first and last column differ, a direction within MARGIN of the seam;
  * 'shadow': a shadow ray whose nearest triangle test passes or fails by less than MARGIN (brute force only);
  * 'dead_margin': mc_shade_ref.dead_rays.
At most CAP of the rows of a case may be exempted (tests/test_relight_cpu.py asserts it for the committed direction sets)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import mc_shade_ref as R

F32, F64 = torch.float32, torch.float64
MARGIN, CAP, K_FLOOR = 1e-5, 0.02, 4.0
MISS_DEPTH = 10.0


# ---- environment lookups ------------------------------------------------------------------------------------------------------------------
def grid_directions(h, w, is_real, dtype=F64):
    """the direction grid of env_light (network/field.py:1021-1034) [h,w,3]: what nero_amd.envlight.latlong_directions computes"""
    az = torch.linspace(1.0, 0.0, w, dtype=F64) * (2 * math.pi) - math.pi / 2
    el = torch.linspace(1.0, -1.0, h, dtype=F64) * (math.pi / 2)
    el, az = torch.meshgrid(el, az, indexing='ij')
    a, b, c = torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)
    return (torch.stack([a, b, c], -1) if is_real else torch.stack([b, c, a], -1)).to(dtype)


def proper_map(h, w, seed=0, hot=None):
    """a random positive map that IS a function of the direction on the project's grid: first and last column equal, pole rows constant;
    hot = (row, column, factor) multiplies one texel"""
    g = torch.Generator().manual_seed(1000 + 31 * h + w + seed)
    env = 0.2 + torch.rand(h, w, 3, generator=g)
    if hot is not None:
        env[hot[0], hot[1]] *= hot[2]
    env[:, -1] = env[:, 0]
    env[0], env[-1] = env[0, 0], env[-1, 0]
    return env.float()


def env_lookup(env, dirs, convention, rot=None, clamp=0.0):
    """env [h,w,3], dirs [n,3] (dtype of dirs rules) -> rgb [n,3], decisions.  The header's nero_env_lookup, formula by formula."""
    dt = dirs.dtype
    env = env.to(dt)
    h, w = env.shape[:2]
    d = dirs if rot is None else dirs @ torch.as_tensor(np.asarray(rot), dtype=dt).reshape(3, 3).T
    dec = {}
    if convention == 2:
        ax = torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
        u = torch.atan2(d[:, 1], -d[:, 0]) / (2 * math.pi) + 0.5
        v = torch.atan2(d[:, 2], ax) / math.pi + 0.5
        x = torch.clamp(u * w - 0.5, -0.5, w - 0.5)
        y = torch.clamp((1 - v) * h - 0.5, 0.0, h - 1.0)
        x0 = torch.floor(x)
        fx = x - x0
        c0, c1 = torch.remainder(x0.long(), w), torch.remainder(x0.long() + 1, w)
    else:
        if convention == 1:
            p, q, up = d[:, 0], d[:, 1], d[:, 2]
        else:
            p, q, up = d[:, 2], d[:, 0], d[:, 1]
        ax = torch.sqrt(p ** 2 + q ** 2)
        az, el = torch.atan2(q, p), torch.atan2(up, ax)
        t = (az + math.pi / 2) / (2 * math.pi)
        t = t - torch.floor(t)
        x = torch.clamp((1 - t) * (w - 1), 0.0, w - 1.0)
        y = torch.clamp((1 - el / (math.pi / 2)) * 0.5 * (h - 1), 0.0, h - 1.0)
        x0 = torch.floor(x)
        fx = x - x0
        c0 = x0.long()
        c1 = torch.clamp(c0 + 1, max=w - 1)
        periodic = bool(torch.equal(env[:, 0], env[:, -1]))
        seam = torch.minimum(t, 1 - t) * (2 * math.pi) * ax / torch.clamp(torch.norm(d, dim=-1), min=1e-30)
        dec['seam'] = (t < 0.5, torch.full_like(seam, 1.0) if periodic else seam)
    y0 = torch.floor(y)
    fy = (y - y0)[:, None]
    r0 = y0.long()
    r1 = torch.clamp(r0 + 1, max=h - 1)
    fx = fx[:, None]
    top = (1 - fx) * env[r0, c0] + fx * env[r0, c1]
    bot = (1 - fx) * env[r1, c0] + fx * env[r1, c1]
    L = (1 - fy) * top + fy * bot
    if clamp > 0:
        L = torch.clamp(L, max=clamp)
    rel = ax / torch.clamp(torch.norm(d, dim=-1), min=1e-30)
    flat = bool((env[0] == env[0, :1]).all()) and bool((env[-1] == env[-1, :1]).all())   # constant pole rows: continuous at the axis
    dec['pole'] = (rel > 0, torch.where((rel == 0) | flat, torch.ones_like(rel), rel))   # exactly on the axis: a tie of direct inputs
    return L, dec


def exempt(dec, keys=('pole', 'seam', 'shadow', 'dead_margin')):
    """[n] bool: rows with a discontinuous decision nearer than MARGIN"""
    out = None
    for k in keys:
        if k in dec:
            dist = dec[k][1]
            e = dist.reshape(dist.shape[0], -1).min(-1)[0] < MARGIN
            out = e if out is None else out | e
    return out


def sample_table(n, dtype=F32):
    """the relighter's direction table [n,2] = (azimuth, elevation) in [0,1]: elevation (j + 0.5) / n -- uniform, which is what makes
    mc_shade_ref.diffuse_dirs cosine-weighted and specular_dirs GGX-distributed -- and azimuth frac(j (sqrt(5) - 1) / 2)"""
    j = torch.arange(n, dtype=F64)
    return torch.stack([torch.remainder(j * ((math.sqrt(5.0) - 1.0) / 2.0), 1.0), (j + 0.5) / n], -1).to(dtype)


# ---- the committed direction set of the lookup tests ----------------------------------------------------------------------------------
def lookup_directions(seed=0, n=2000):
    """the committed direction set of the lookup tests: random directions of any length, the six axes (both poles of every convention), the
    seams, grid points of a 5 x 7 map"""
    g = torch.Generator().manual_seed(77 + seed)
    rnd = torch.randn(n, 3, generator=g) * (0.2 + 2 * torch.rand(n, 1, generator=g))
    axes = torch.cat([torch.eye(3), -torch.eye(3)])
    t = torch.linspace(-1.2, 1.2, 9)
    seams = torch.cat([torch.stack([torch.cos(t), torch.zeros_like(t), torch.sin(t)], -1),      # convention 2 (u = 0 | 1) at +x
                       torch.stack([torch.zeros_like(t), -torch.cos(t), torch.sin(t)], -1),     # convention 1: az = -pi / 2
                       torch.stack([-torch.cos(t), torch.sin(t), torch.zeros_like(t)], -1)])    # convention 0: az = -pi / 2
    grid = torch.cat([grid_directions(5, 7, r, torch.float32).reshape(-1, 3) for r in (0, 1)])
    return torch.cat([rnd, axes, seams, grid]).float().contiguous()


ROT = np.asarray([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)


# ---- relighting -----------------------------------------------------------------------------------------------------------------------------
def relight(pt, w, blocked, dead, env, convention, rot, clamp, Dd, Ds, geometry_type):
    """pt [P,32], w [P D,3], blocked / dead [P D] bool -> rgb_lin, diffuse_lin, spec_lin [P,3], decisions: shade_mixed (mc_shade_ref.
    estimator) with L = the environment's radiance where the shadow ray is free and the direction not dead, else 0"""
    P_, D = pt.shape[0], Dd + Ds
    L, dec = env_lookup(env, w, convention, rot, clamp)
    L = torch.where((blocked | dead)[:, None], torch.zeros_like(L), L)
    rgb, _, _, spec, dec_e = R.estimator(pt, pt[:, None, 9:14], w.reshape(P_, D, 3), L.reshape(P_, D, 3), Dd, Ds, geometry_type)
    dec = {k: (s.reshape(P_, D), m.reshape(P_, D)) for k, (s, m) in dec.items()}
    dec.update(dec_e)
    return rgb, rgb - spec, spec, dec


def floors_and_errors(got, ref32, ref64, scale):
    """per row: the float32 floor |ref32 - ref64| and the kernel's distance |got - ref64|, both relative to max(|ref64|, scale) -> [P], [P]"""
    den = torch.clamp(ref64.abs(), min=scale)
    return ((ref32.double() - ref64).abs() / den).max(-1)[0], ((got.double() - ref64).abs() / den).max(-1)[0]


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------
def interpolate(attr, tris, face, bary):
    """attr [V,C], tris [T,3], face [n] (>= 0), bary [n,2] = (u, v) -> (1 - u - v) a0 + u a1 + v a2"""
    f = tris.long()[face.long()]
    u, v = bary[:, 0:1].to(attr.dtype), bary[:, 1:2].to(attr.dtype)
    return (1 - u - v) * attr[f[:, 0]] + u * attr[f[:, 1]] + v * attr[f[:, 2]]


def closest_hit(V, Fc, o, d, tmax=MISS_DEPTH, chunk=1024):
    """brute force over all triangles with the tracer's own predicates (Moeller-Trumbore: |det| >= 1e-20, 0 <= u <= 1, v >= 0, u + v <= 1,
    0 < t < best) in the dtype of o -> depth [n] (tmax: miss), face [n] (-1: miss), bary [n,2], margin [n]: the smallest distance of any
    nearer-than-the-hit triangle's (u, v, u + v, t) from its bounds -- how far the answer is from changing"""
    dt = o.dtype
    V, Fc = V.to(dt), Fc.long()
    v0 = V[Fc[:, 0]][None]
    e1, e2 = V[Fc[:, 1]][None] - v0, V[Fc[:, 2]][None] - v0
    out = []
    for i in range(0, o.shape[0], chunk):
        oo, dd = o[i:i + chunk, None], d[i:i + chunk, None]
        pv = torch.linalg.cross(dd.expand(-1, e2.shape[1], -1), e2.expand(dd.shape[0], -1, -1))
        det = (e1 * pv).sum(-1)
        inv = 1.0 / torch.where(det.abs() < 1e-20, torch.ones_like(det), det)
        tv = oo - v0
        u = (tv * pv).sum(-1) * inv
        qv = torch.linalg.cross(tv, e1.expand(tv.shape[0], -1, -1))
        v = (dd * qv).sum(-1) * inv
        t = (e2 * qv).sum(-1) * inv
        ok = (det.abs() >= 1e-20) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < tmax)
        tt = torch.where(ok, t, torch.full_like(t, tmax))
        depth, face = tt.min(-1)
        hit = depth < tmax
        inside = torch.minimum(torch.minimum(u, v), 1 - u - v)                       # > 0 inside, < 0 outside
        near = (t > 0) & (t < tmax) & (det.abs() >= 1e-20)
        margin = torch.where(near, inside.abs(), torch.full_like(inside, 1.0)).min(-1)[0]
        idx = torch.arange(face.shape[0])
        bary = torch.stack([u[idx, face], v[idx, face]], -1)
        out.append((depth, torch.where(hit, face, torch.full_like(face, -1)), torch.where(hit[:, None], bary, torch.zeros_like(bary)), margin))
    return tuple(torch.cat(x) for x in zip(*out))


def occluded(V, Fc, o, d, tmax=MISS_DEPTH):
    """-> blocked [n] bool, decisions {'shadow'}"""
    depth, _, _, margin = closest_hit(V, Fc, o, d, tmax)
    return depth < tmax, {'shadow': (depth < tmax, margin)}


def scene(subdiv=3, quad=True):
    """icosphere of radius 0.5 (nero_amd.synthetic.icosphere) plus a small quad occluder above it (two triangles at z = 0.8, half-width 0.2)
    -> V [nV,3] float32, F [nT,3] int64 (torch)"""
    from nero_amd.synthetic import icosphere
    v, f = icosphere(subdiv, 0.5)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int64)
    if quad:
        q = np.asarray([[-0.2, -0.2, 0.8], [0.2, -0.2, 0.8], [0.2, 0.2, 0.8], [-0.2, 0.2, 0.8]], np.float32)
        f = np.concatenate([f, np.asarray([[0, 1, 2], [0, 2, 3]]) + len(v)])
        v = np.concatenate([v, q])
    return torch.from_numpy(v), torch.from_numpy(f)


# ---- cameras --------------------------------------------------------------------------------------------------------------------------------
def relighting_poses(num, azimuth, elevation, dist):
    """the relighting orbit [num,3,4] float64: cameras on half a turn about the z axis around `azimuth` (degrees) at `elevation` (degrees),
    looking at the origin with z up, in a world turned by 90 degrees about x; translation (0, 0, dist)"""
    az = math.radians(azimuth) + torch.linspace(-math.pi / 2, math.pi / 2, num, dtype=F64)
    el = torch.full_like(az, math.radians(elevation))
    cam = torch.stack([torch.cos(az) * torch.cos(el), torch.sin(az) * torch.cos(el), torch.sin(el)], -1)
    z = F.normalize(-cam, dim=-1)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=F64)
    y = -F.normalize(up[None] - (z * up[None]).sum(-1, keepdim=True) * z, dim=-1)
    x = torch.linalg.cross(y, z)
    rot = torch.stack([x, y, z], 1) @ torch.tensor([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=F64)
    t = torch.tensor([0.0, 0.0, float(dist)], dtype=F64).expand(num, 3)[..., None]
    return torch.cat([rot, t], -1)


def camera_rays(pose, K, h, w, dtype=F64):
    """pixel centres + 0.5 through K and the world-to-camera pose -> rays_o, rays_d [h w,3]"""
    pose, K = torch.as_tensor(np.asarray(pose), dtype=dtype), torch.as_tensor(np.asarray(K), dtype=dtype)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    c = torch.stack([xs + 0.5, ys + 0.5, torch.ones_like(xs, dtype=dtype)], -1).reshape(-1, 3).to(dtype)
    d = F.normalize((c @ torch.inverse(K).T) @ pose[:, :3], dim=-1)
    o = (-pose[:, :3].T @ pose[:, 3:]).T.expand(h * w, 3)
    return o.contiguous(), d.contiguous()
