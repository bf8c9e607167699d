"""Relighting of the Stage-II mesh under an HDR environment map on the GPU: what the reference's relight.py hands to Blender Cycles, as
direct lighting with shadows on the mesh tracer's BVH (include/nero_hip_relight.h, nero_amd/csrc/relight.hip).

Camera rays go through nero_bvh_trace_faces (depth, face, barycentrics), the per-vertex materials are interpolated at the hits, and
nero_bvh_relight evaluates the reference's shade_mixed estimator with "environment radiance if the shadow ray is free, zero if it is
blocked" for the light -- one fused kernel that never stores a ray.  With bounces=1 a blocked direction is not black: it fetches the light
the surface it meets sends back under its own direct lighting (one bounce, one sample, a shadow ray of its own; include/nero_hip_bounce.h,
DESIGN.md 9.12.2).  Smooth shading takes per-vertex normals, the caller's or computed here (normals='angle' / 'area').  render(denoise=True)
filters the noise a sample count leaves with a single-frame edge-aware filter (nero_amd/denoise.py).
Relighter(textures=...) reads the materials from the UV maps bake_materials writes instead of per vertex, through a mip pyramid with a
trilinear fetch (nero_amd/texfetch.py).  NOT modelled: more than one bounce, textures at secondary hits.
This is not Cycles.

samples = (Dd, Ds) draws every direction from the BRDF; samples = (Dd, Ds, Dl) adds Dl directions drawn from the map itself (light_table,
nero_env_cdf) and weighs all of them by one mixture density in nero_bvh_relight_mis (include/nero_hip_envsample.h): the
same expectation, far less noise under a map with a sun or a lamp in it.

ROUGHNESS: extract_materials.py stores -- and predict_materials_of_vertices returns -- the PERCEPTUAL roughness (the square root of what
the network predicts); the estimator takes alpha = roughness^2.  Everything here carries the perceptual value, as a renderer's vertex
attribute would, and estimator_materials() below squares it: the one place."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib as L
from .raytracing import RayTracer
from .renderer import linear_to_srgb
from .texture import _png_chunk

CONVENTIONS = {'nero': 0, 'nero_real': 1, 'blender': 2}          # nero_env_lookup's `convention`
GEOMETRY_TYPES = {'schlick': 0, 'ggx_smith': 1}                  # as nero_amd.stage2
NORMAL_MODES = ('angle', 'area')                                 # Relighter(normals=...): vertex normals computed from the mesh
MISS_DEPTH = 10.0
MAX_LANES = 2 ** 31 - 64                                         # (point, padded sample) lanes of one nero_bvh_relight call
DEFAULT_CHUNK_LANES = 1 << 26


_lib = L.lib


# ---- cameras --------------------------------------------------------------------------------------------------------------------------------
def relighting_poses(num, azimuth, elevation, dist):
    """the orbit of the reference's generate_relghting_poses (blender_backend/blender_utils.py:101-116): `num` world-to-camera poses [num,3,4]
    (float64) on half a turn around the azimuth (degrees) at one elevation (degrees), every camera looking at the origin from `dist`; the
    object frame is turned by 90 degrees about x against the camera orbit's (R_trans), as there"""
    az = np.deg2rad(azimuth) + np.linspace(-np.pi / 2, np.pi / 2, num)
    el = np.ones_like(az) * np.deg2rad(elevation)
    cam = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1)
    up = np.asarray([0.0, 0.0, 1.0])
    z = -cam / np.linalg.norm(cam, axis=1, keepdims=True)
    y = -(up[None] - np.sum(z * up[None], 1, keepdims=True) * z)
    y = y / np.linalg.norm(y, axis=1, keepdims=True)
    x = np.cross(y, z)
    rot = np.stack([x, y, z], 1) @ np.asarray([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])[None]
    t = np.repeat(np.asarray([0.0, 0.0, float(dist)])[None, :, None], num, 0)
    return np.concatenate([rot, t], -1)


R_BLENDER = np.asarray([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])       # x_blender = R_BLENDER x_world (blender_utils.set_camera_by_pose)


def poses_in_mesh_frame(poses):
    """the poses of relighting_poses as cameras over the mesh's OWN coordinates.  The reference imports the mesh into Blender untouched and
    places the camera of a pose [R | t] at rotation R R_BLENDER^T (set_camera_by_pose): Blender's frame is the mesh's, and the turn inside
    the poses (R_trans = R_BLENDER) cancels -- the cameras orbit the mesh's z axis, z up.  [n,3,4] -> [n,3,4]"""
    poses = np.asarray(poses, np.float64)
    return np.concatenate([poses[:, :, :3] @ R_BLENDER.T[None], poses[:, :, 3:]], -1)


def default_K(h, w):
    """Blender's default camera (50 mm lens on a 36 mm sensor) for an h x w image: focal w 50 / 36, principal point at the centre"""
    f = w * 50.0 / 36.0
    return np.asarray([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]], np.float32)


# ---- materials ------------------------------------------------------------------------------------------------------------------------------
def load_materials(path):
    """metallic.npy [V,1], roughness.npy [V,1] (PERCEPTUAL, as stored), albedo.npy [V,3] of a directory extract_materials.py wrote -> the
    dict predict_materials_of_vertices returns.  Nothing is squared here (estimator_materials does that)."""
    out = {k: np.asarray(np.load(os.path.join(path, k + '.npy')), np.float32) for k in ('metallic', 'roughness', 'albedo')}
    n = out['albedo'].shape[0]
    out['metallic'], out['roughness'], out['albedo'] = out['metallic'].reshape(n, 1), out['roughness'].reshape(n, 1), out['albedo'].reshape(n, 3)
    return out


def estimator_materials(mat5):
    """[n,5] (metallic, PERCEPTUAL roughness, albedo) -> [n,5] (metallic, alpha = roughness^2, albedo): THE place where the stored roughness
    is squared, once, for the estimator (nero_mc_point_setup's mat5)"""
    return torch.cat([mat5[:, 0:1], mat5[:, 1:2] * mat5[:, 1:2], mat5[:, 2:5]], -1)


# ---- RGBA PNG -------------------------------------------------------------------------------------------------------------------------------
def rgba_png_bytes(img):
    """uint8 [h, w, 4] -> the bytes of a non-interlaced 8-bit RGBA PNG (colour type 6, filter 0 on every row; straight alpha)"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f'rgba_png_bytes: [h, w, 4] expected, got {img.shape}')
    h, w = img.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, -1)], 1)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 6, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', ihdr) + _png_chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _png_chunk(b'IEND', b'')


def write_rgba_png(path, img):
    if torch.is_tensor(img):
        img = img.detach().cpu().numpy()
    with open(path, 'wb') as fh:
        fh.write(rgba_png_bytes(img))


# ---- sample tables, hashes ------------------------------------------------------------------------------------------------------------------
def sample_table(n, device=None):
    """the relighter's (azimuth, elevation) table of n directions in [0,1]^2, float32 [n,2]: elevation (j + 0.5) / n, azimuth frac(j (sqrt(5)
    - 1) / 2) -- a golden-ratio lattice.  sample_diffuse_directions reads the elevation as sin^2(theta) and sample_specular_directions as
    the uniform variate of the GGX lobe, so a table UNIFORM in elevation makes the first cosine-weighted and the second GGX-distributed, as
    the estimator's densities assume.  The training tables (network/field.py:741-749: 1 - 2 arcsin(z) / pi over a Fibonacci sphere) are not
    uniform in it -- the mean of a constant light is still the light, but a half-blocked hemisphere is weighed wrongly -- so they are not
    used here."""
    j = np.arange(n, dtype=np.float64)
    tab = np.stack([np.mod(j * ((np.sqrt(5.0) - 1.0) / 2.0), 1.0), (j + 0.5) / n], -1).astype(np.float32)
    out = torch.from_numpy(tab).contiguous()
    return out if device is None else out.to(device)


def _lowbias32(x):
    m = 0xffffffff
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & m
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & m
    return x ^ (x >> 16)


def pixel_rotations(index, seed):
    """two azimuth rotations in [0,1) per pixel from a counter hash of (pixel index, seed) -- a function of the pixel alone, so the same for
    every chunking: h1 = lowbias32(index 0x9E3779B9 + seed), h2 = lowbias32(h1 + 0x68E31DA4), r = (h >> 8) 2^-24.  index: int64 tensor"""
    m = 0xffffffff
    h1 = _lowbias32((index.long() * 0x9E3779B9 + (int(seed) & m)) & m)
    h2 = _lowbias32((h1 + 0x68E31DA4) & m)
    return (h1 >> 8).float() * 2.0 ** -24, (h2 >> 8).float() * 2.0 ** -24


def pixel_shifts(index, seed):
    """the two shifts in [0,1) of a pixel's light samples: two more hashes chained after pixel_rotations' h2 by the same step, h3 =
    lowbias32(h2 + 0x68E31DA4), h4 = lowbias32(h3 + 0x68E31DA4), s = (h >> 8) 2^-24 -> [n,2] float32.  index: int64 tensor"""
    m = 0xffffffff
    h1 = _lowbias32((index.long() * 0x9E3779B9 + (int(seed) & m)) & m)
    h2 = _lowbias32((h1 + 0x68E31DA4) & m)
    h3 = _lowbias32((h2 + 0x68E31DA4) & m)
    h4 = _lowbias32((h3 + 0x68E31DA4) & m)
    return torch.stack([(h3 >> 8).float() * 2.0 ** -24, (h4 >> 8).float() * 2.0 ** -24], -1)


def pixel_keys(index, seed):
    """the key of a pixel's bounces: one more hash chained after pixel_shifts' h4 by the same step, h5 = lowbias32(h4 + 0x68E31DA4) -> [n]
    int64 in [0, 2^32) (relight_points sends it as uint32).  The variates of sample j's bounce are hashes of (key, j): a function of (pixel,
    seed, j) alone, so the same for every chunking.  index: int64 tensor"""
    m = 0xffffffff
    h = _lowbias32((index.long() * 0x9E3779B9 + (int(seed) & m)) & m)
    for _ in range(4):
        h = _lowbias32((h + 0x68E31DA4) & m)
    return h


def padded_samples(Dd, Ds, Dl=0):
    return (Dd + Ds + Dl + 63) // 64 * 64


# ---- thin wrappers of the entry points ------------------------------------------------------------------------------------------------------
def _rot_arg(rot):
    if rot is None:
        return None
    r = np.asarray(rot.detach().cpu().numpy() if torch.is_tensor(rot) else rot, np.float32).reshape(9)
    return (C.c_float * 9)(*[float(x) for x in r])


def export_faces(tracer):
    """leaf slot -> face index of the tracer's tree, int32 numpy [n_tris] (nero_bvh_export_faces)"""
    n = tracer.info()['n_tris']
    out = np.empty(n, np.int32)
    L.check(_lib.nero_bvh_export_faces(tracer._handle(), out.ctypes.data_as(C.c_void_p)))
    return out


def trace_faces(tracer, rays_o, rays_d):
    """closest hit with the face (nero_bvh_trace_faces): rays [n,3] CUDA float32 -> depth [n] (10: miss), face [n] int32 (-1: miss), bary [n,2]"""
    rays_o, rays_d = rays_o.float().contiguous(), rays_d.float().contiguous()
    n = rays_o.shape[0]
    depth = torch.empty(n, dtype=torch.float32, device=rays_o.device)
    face = torch.empty(n, dtype=torch.int32, device=rays_o.device)
    bary = torch.empty(n, 2, dtype=torch.float32, device=rays_o.device)
    with torch.cuda.device(rays_o.device):
        L.check(_lib.nero_bvh_trace_faces(tracer._handle(), L.ptr(rays_o), L.ptr(rays_d), n, L.ptr(depth), L.ptr(face), L.ptr(bary), L.stream_ptr()))
    return depth, face, bary


def env_lookup(env, dirs, convention=2, rot=None, clamp=None):
    """bilinear radiance of the lat-long map env [h,w,3] in the directions dirs [n,3] (nero_env_lookup) -> [n,3]"""
    env, dirs = env.float().contiguous(), dirs.float().contiguous()
    n = dirs.shape[0]
    out = torch.empty(n, 3, dtype=torch.float32, device=dirs.device)
    with torch.cuda.device(dirs.device):
        L.check(_lib.nero_env_lookup(L.ptr(env), env.shape[0], env.shape[1], int(CONVENTIONS.get(convention, convention)), _rot_arg(rot),
                                     L.ptr(dirs), n, float(clamp or 0.0), L.ptr(out), L.stream_ptr()))
    return out


def relight_rays(pt, tab_d, tab_s, geometry_type=0):
    """the sample set of relight_points (nero_relight_rays) -> rays_o, rays_d [P D,3], dead [P D] uint8"""
    P, Dd, Ds = pt.shape[0], tab_d.shape[0], tab_s.shape[0]
    n = P * (Dd + Ds)
    ro = torch.empty(n, 3, dtype=torch.float32, device=pt.device)
    rd = torch.empty_like(ro)
    dead = torch.empty(n, dtype=torch.uint8, device=pt.device)
    with torch.cuda.device(pt.device):
        L.check(_lib.nero_relight_rays(L.ptr(pt), L.ptr(tab_d), L.ptr(tab_s), P, Dd, Ds, int(geometry_type), L.ptr(ro), L.ptr(rd), L.ptr(dead),
                                       L.stream_ptr()))
    return ro, rd, dead


class LightTable:
    """the sampling table of one map under one convention, rotation and cap (nero_env_cdf): cdf [gh gw] int64, info [5] int64 = (total,
    zero-weight cells, e, B, fallback), both on the device; weights [gh gw] float32 when asked for"""

    def __init__(self, cdf, info, gh, gw, weights=None):
        self.cdf, self.info, self.gh, self.gw, self.weights = cdf, info, int(gh), int(gw), weights


def light_table(env, convention=2, rot=None, clamp=None, weights=False):
    """env [h,w,3] CUDA -> LightTable: luminance x cos(elevation) per cell of an h x w equirectangular grid in world directions, as integer
    weights and their running sum (include/nero_hip_envsample.h)"""
    env = env.float().contiguous()
    gh, gw = int(env.shape[0]), int(env.shape[1])
    dev = env.device
    with torch.cuda.device(dev):
        need = int(_lib.nero_env_cdf_workspace_bytes(gh, gw))
        if need == 0:
            raise L.NeroHipError(_lib.nero_last_error().decode())
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        cdf = torch.empty(gh * gw, dtype=torch.int64, device=dev)
        info = torch.empty(5, dtype=torch.int64, device=dev)
        wts = torch.empty(gh * gw, dtype=torch.float32, device=dev) if weights else None
        L.check(_lib.nero_env_cdf(L.ptr(env), gh, gw, int(CONVENTIONS.get(convention, convention)), _rot_arg(rot), float(clamp or 0.0), L.ptr(ws),
                                  L.ptr(cdf), L.ptr(info), L.ptr(wts), L.stream_ptr()))
    return LightTable(cdf, info, gh, gw, wts)


def relight_mis_rays(pt, tab_d, tab_s, tab_l, table, rand_l=None, geometry_type=0):
    """the sample set of the three strategies (nero_relight_mis_rays) -> rays_o, rays_d [P D,3], dead [P D] uint8, cell [P D] int32,
    pdf_l [P D]; D = Dd + Ds + Dl, cosine then GGX then light samples"""
    P, Dd, Ds, Dl = pt.shape[0], tab_d.shape[0], tab_s.shape[0], tab_l.shape[0]
    n = P * (Dd + Ds + Dl)
    ro = torch.empty(n, 3, dtype=torch.float32, device=pt.device)
    rd = torch.empty_like(ro)
    dead = torch.empty(n, dtype=torch.uint8, device=pt.device)
    cell = torch.empty(n, dtype=torch.int32, device=pt.device)
    pdf = torch.empty(n, dtype=torch.float32, device=pt.device)
    rl = None if rand_l is None else rand_l.float().contiguous()
    with torch.cuda.device(pt.device):
        L.check(_lib.nero_relight_mis_rays(L.ptr(pt), L.ptr(tab_d), L.ptr(tab_s), L.ptr(tab_l), L.ptr(rl), P, Dd, Ds, Dl, int(geometry_type),
                                           L.ptr(table.cdf), L.ptr(table.info), table.gh, table.gw, L.ptr(ro), L.ptr(rd), L.ptr(dead),
                                           L.ptr(cell), L.ptr(pdf), L.stream_ptr()))
    return ro, rd, dead, cell, pdf


def _mesh_args(mesh, dev):
    """(verts, tris int32, mat5 PERCEPTUAL, normals | None) -> contiguous device tensors of the types the bounce entry points read"""
    if mesh is None or len(mesh) != 4:
        raise ValueError('bounces=1 needs mesh=(verts [V,3], tris [T,3] int32, mat5 [V,5] with the perceptual roughness, normals [V,3] or None)')
    verts, tris, mat5, normals = mesh
    verts, mat5 = verts.to(dev, torch.float32).contiguous(), mat5.to(dev, torch.float32).contiguous()
    tris = tris.to(dev, torch.int32).contiguous()
    normals = None if normals is None else normals.to(dev, torch.float32).contiguous()
    assert verts.ndim == 2 and verts.shape[1] == 3 and tris.ndim == 2 and tris.shape[1] == 3 and tuple(mat5.shape) == (verts.shape[0], 5)
    assert normals is None or normals.shape == verts.shape
    return verts, tris, mat5, normals


def _key_arg(key, P, dev):
    """[P] integers in [0, 2^32) -> the same bits as int32 on the device (read as uint32), or None"""
    if key is None:
        return None
    k = key.to(dev).long() & 0xffffffff
    assert k.shape == (P,), k.shape
    return torch.where(k >= 2 ** 31, k - 2 ** 32, k).to(torch.int32).contiguous()


def relight_bounce_rays(tracer, pt, tab_d, tab_s, mesh, key=None, geometry_type=0, tab_l=None, rand_l=None, table=None):
    """what every lane of the bounce kernels decides (nero_relight_bounce_rays) -> dict: state [P D] uint8 (0 free, 1 dead, 2 bounced, 3
    bounced with a dead secondary sample, 4 bad face), face [P D] int32, bary [P D,2], sec_o, sec_d [P D,3], strategy [P D] int32, pdf_l
    [P D], cell [P D] int32.  tab_l and table: the MIS variant"""
    dev = pt.device
    P, Dd, Ds, Dl = pt.shape[0], tab_d.shape[0], tab_s.shape[0], 0 if tab_l is None else tab_l.shape[0]
    n = P * (Dd + Ds + Dl)
    verts, tris, mat5, normals = _mesh_args(mesh, dev)
    kk = _key_arg(key, P, dev)
    out = {'state': torch.empty(n, dtype=torch.uint8, device=dev), 'face': torch.empty(n, dtype=torch.int32, device=dev),
           'bary': torch.empty(n, 2, dtype=torch.float32, device=dev), 'sec_o': torch.empty(n, 3, dtype=torch.float32, device=dev),
           'sec_d': torch.empty(n, 3, dtype=torch.float32, device=dev), 'strategy': torch.empty(n, dtype=torch.int32, device=dev),
           'pdf_l': torch.empty(n, dtype=torch.float32, device=dev), 'cell': torch.empty(n, dtype=torch.int32, device=dev)}
    rl = None if rand_l is None else rand_l.float().contiguous()
    tl = (None, None, 1, 1) if tab_l is None else (L.ptr(table.cdf), L.ptr(table.info), table.gh, table.gw)
    with torch.cuda.device(dev):
        L.check(_lib.nero_relight_bounce_rays(tracer._handle(), L.ptr(pt), L.ptr(tab_d), L.ptr(tab_s), L.ptr(tab_l), L.ptr(rl), P, Dd, Ds, Dl,
                                              int(geometry_type), *tl, L.ptr(verts), verts.shape[0], L.ptr(tris), tris.shape[0], L.ptr(mat5),
                                              L.ptr(normals), L.ptr(kk), *[L.ptr(out[k]) for k in ('state', 'face', 'bary', 'sec_o', 'sec_d',
                                                                                                   'strategy', 'pdf_l', 'cell')], L.stream_ptr()))
    return out


def relight_points(tracer, pt, tab_d, tab_s, env, convention=2, rot=None, clamp=None, geometry_type=0, chunk=None, tab_l=None, rand_l=None,
                   table=None, bounces=0, mesh=None, key=None):
    """the fused kernel (nero_bvh_relight) over the point records pt [P,32], in chunks of `chunk` points (None: as many as fit
    DEFAULT_CHUNK_LANES lanes; always within the per-call limit) -> rgb_lin, diffuse_lin, spec_lin [P,3].  Same bits for every chunk.
    With tab_l [Dl,2]: the MIS kernel (nero_bvh_relight_mis) with Dl light samples per point drawn from `table` (a LightTable of this map,
    convention, rotation and cap; None: built here), shifted per point by rand_l [P,2] (None: no shift).
    bounces=1: the bounce kernels (nero_bvh_relight_bounce / nero_bvh_relight_mis_bounce) over mesh = (verts [V,3], tris [T,3] int32, mat5
    [V,5] with the PERCEPTUAL roughness, normals [V,3] or None) -- the arrays the tracer's tree was built from -- with key [P] (pixel_keys;
    None: zeros) seeding each point's bounces -> rgb_lin, diffuse_lin, spec_lin (the direct terms: bounces=0's bits), indirect_lin."""
    if bounces not in (0, 1):
        raise ValueError(f'bounces {bounces!r}: 0 (direct lighting) or 1 (one inter-reflection)')
    return _relight_chunks(tracer, pt, tab_d, tab_s, tab_l, rand_l, table, env, convention, rot, clamp, geometry_type, chunk, bounces, mesh, key)


# (MIS, bounces) -> the fused entry point and the one that sizes its workspace
_FUSED = {(False, 0): (_lib.nero_bvh_relight, _lib.nero_relight_workspace_bytes),
          (True, 0): (_lib.nero_bvh_relight_mis, _lib.nero_relight_mis_workspace_bytes),
          (False, 1): (_lib.nero_bvh_relight_bounce, _lib.nero_relight_bounce_workspace_bytes),
          (True, 1): (_lib.nero_bvh_relight_mis_bounce, _lib.nero_relight_mis_bounce_workspace_bytes)}


def _relight_chunks(tracer, pt, tab_d, tab_s, tab_l, rand_l, table, env, convention, rot, clamp, geometry_type, chunk, bounces, mesh, key):
    """relight_points' work: slices of `chunk` points through one fused entry point -- tab_l picks the MIS ones, bounces the bounce ones --
    into one workspace -> rgb_lin, diffuse_lin, spec_lin [P,3], and indirect_lin with bounces"""
    mis = tab_l is not None
    fused, sizer = _FUSED[mis, bounces]
    P, Dd, Ds, Dl = pt.shape[0], tab_d.shape[0], tab_s.shape[0], tab_l.shape[0] if mis else 0
    counts = (Dd, Ds, Dl) if mis else (Dd, Ds)
    pad = padded_samples(Dd, Ds, Dl)
    most = max(1, MAX_LANES // pad)
    chunk = max(1, DEFAULT_CHUNK_LANES // pad) if chunk is None else int(chunk)
    chunk = max(1, min(chunk, most))
    dev = pt.device
    out = [torch.zeros(P, 3, dtype=torch.float32, device=dev) for _ in range(4 if bounces else 3)]
    env = env.float().contiguous()
    conv, rot_arg = int(CONVENTIONS.get(convention, convention)), _rot_arg(rot)
    if bounces:
        verts, tris, mat5, normals = _mesh_args(mesh, dev)
        mesh_args = (L.ptr(verts), verts.shape[0], L.ptr(tris), tris.shape[0], L.ptr(mat5), L.ptr(normals))
        kk = _key_arg(key, P, dev)
    if mis and table is None:
        table = light_table(env, conv, rot, clamp)
    if mis:
        assert (table.gh, table.gw) == tuple(env.shape[:2]), 'the light table is not this map\'s'
    rl = None if rand_l is None else rand_l.float().contiguous()
    env_args = (L.ptr(env), env.shape[0], env.shape[1], conv, rot_arg, float(clamp or 0.0)) + ((L.ptr(table.cdf), L.ptr(table.info)) if mis else ())
    with torch.cuda.device(dev):
        need = int(sizer(min(chunk, max(P, 1)), *counts))
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        for i in range(0, P, chunk):
            at = slice(i, i + min(chunk, P - i))
            light = (L.ptr(tab_l), None if rl is None else L.ptr(rl[at])) if mis else ()
            scene = (*mesh_args, None if kk is None else L.ptr(kk[at])) if bounces else ()
            L.check(fused(tracer._handle(), L.ptr(pt[at]), L.ptr(tab_d), L.ptr(tab_s), *light, at.stop - i, *counts, int(geometry_type), *env_args,
                          *scene, *[L.ptr(o[at]) for o in out], L.ptr(ws), ws.numel(), L.stream_ptr()))
    return tuple(out)


def point_records(pts, view, normals, mat5, rand_d, rand_s):
    """nero_mc_point_setup -> pt [P,32]; mat5 carries alpha (estimator_materials)"""
    P = pts.shape[0]
    pt = torch.empty(P, 32, dtype=torch.float32, device=pts.device)
    args = [t.float().contiguous() for t in (pts, view, normals, mat5)]
    rd = None if rand_d is None else rand_d.float().contiguous()
    rs = None if rand_s is None else rand_s.float().contiguous()
    with torch.cuda.device(pts.device):
        L.check(_lib.nero_mc_point_setup(*[L.ptr(t) for t in args], L.ptr(rd), L.ptr(rs), P, L.ptr(pt), L.stream_ptr()))
    return pt


# ---- the relighter --------------------------------------------------------------------------------------------------------------------------
class Relighter:
    """verts [V,3], tris [T,3]; materials: {'metallic' [V,1], 'roughness' [V,1] PERCEPTUAL, 'albedo' [V,3]} (load_materials,
    predict_materials_of_vertices); env: linear radiance [h,w,3] (array, tensor) or the path of a Radiance .hdr; convention: 'blender'
    (the equirectangular mapping of an .hdr made for relight.py --hdr), 'nero' / 'nero_real' (this project's env_light grid, is_real = 0 /
    1); env_rotation: 3 x 3, applied to a direction before the lookup; tracer: a RayTracer over the same mesh to share, else one is built
    (`build`); normals: per-vertex [V,3] for smooth shading, 'angle' or 'area' to compute them from the mesh (nero_amd.mesh.vertex_normals,
    stored outward; the flat normal stands in wherever one has no direction), else flat face normals turned towards the camera; bounces:
    render()'s default.
    textures: None, or the dict read_textured_obj or bake_materials returns -- 'albedo' uint8 [h,w,3], 'metallic', 'roughness' uint8 [h,w]
    (every channel sRGB-encoded, the roughness channel holding alpha), 'vt' [Vt,2], 'ft' [T,3] -- and `materials` may then be None: the
    camera's hits take their materials from the maps, filtered to the pixel's footprint (nero_amd/texfetch.py);
    lod_bias shifts the level of detail (+1: one level blurrier).  self.mat5 is then texfetch.vertex_materials: one level-0 fetch per
    vertex, which is what the bounce kernels shade the surface at a SECONDARY hit from -- an approximation: a bounce sees the maps at
    the vertex spacing.  Without textures nothing changes.
    normal_map: None, or the dict nero_amd.transfer.bake_normal_map returns -- 'normal' uint8 [h,w,3], 'vt' [Vt,2], 'ft' [T,3], optional
    'space' ('tangent', the default, or 'object') -- independent of textures: surface() perturbs its normal with the map (the fused
    lookup of nero_amd/transfer.py, filtered to the pixel's footprint like the materials) just before normalising, so
    the estimator and the denoiser's guides see the detailed normal.  A tangent-space map wants the frame it was baked in: pass the same
    `normals` mode (the bake's result records it).  Secondary hits of bounces=1 keep the per-vertex normals: an approximation, like the
    textures there.  Without normal_map nothing changes."""

    def __init__(self, verts, tris, materials, env, convention='blender', env_rotation=None, tracer=None, build='device',
                 geometry_type='schlick', normals=None, device=None, bounces=0, textures=None, lod_bias=0.0, normal_map=None):
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        as_t = lambda a, dt: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
        self.device = dev
        self.verts, self.tris = as_t(verts, torch.float32).reshape(-1, 3), as_t(tris, torch.int64).reshape(-1, 3)
        V = self.verts.shape[0]
        self.textures, self.lod_bias = None, float(lod_bias)
        if textures is not None:
            from . import texfetch
            self.textures = texfetch.TextureSet(textures['albedo'], textures['metallic'], textures['roughness'], device=dev)
            self.vt, self.ft = as_t(textures['vt'], torch.float32).reshape(-1, 2), as_t(textures['ft'], torch.int32).reshape(-1, 3)
            if self.ft.shape != self.tris.shape:
                raise ValueError(f'textures: ft has {self.ft.shape[0]} faces, the mesh {self.tris.shape[0]}')
            self.face_scale = texfetch.face_scale(self.verts, self.tris.int(), self.vt, self.ft, self.textures.h, self.textures.w)
            self.mat5 = texfetch.vertex_materials(self.textures, self.vt, self.tris.int(), self.ft, V)       # the bounce kernels' stand-in
        else:
            self.mat5 = torch.cat([as_t(materials[k], torch.float32).reshape(V, -1) for k in ('metallic', 'roughness', 'albedo')], -1)   # perceptual
        assert self.mat5.shape[1] == 5, self.mat5.shape
        self.normal_map = None
        if normal_map is not None:                                      # pyramid, texel density, tangents and signs: once
            from . import texfetch, transfer
            self.normal_map = transfer.NormalMap(normal_map['normal'], normal_map.get('space', 'tangent'), device=dev)
            self.nm_vt, self.nm_ft = as_t(normal_map['vt'], torch.float32).reshape(-1, 2), as_t(normal_map['ft'], torch.int32).reshape(-1, 3)
            if self.nm_ft.shape != self.tris.shape:
                raise ValueError(f'normal_map: ft has {self.nm_ft.shape[0]} faces, the mesh {self.tris.shape[0]}')
            self.nm_scale = texfetch.face_scale(self.verts, self.tris.int(), self.nm_vt, self.nm_ft, self.normal_map.h, self.normal_map.w)
            self.nm_tangent, self.nm_sign = transfer.uv_tangents(self.verts, self.tris.int(), self.nm_vt, self.nm_ft)
        # 'angle' / 'area': smooth normals computed here, once, and stored OUTWARD whatever the winding (the bounce kernels read them at
        # secondary hits without turning them); where they fail (zero, not finite) surface() falls back to the flat normal
        self._computed_normals = isinstance(normals, str)
        if self._computed_normals:
            if normals not in NORMAL_MODES:
                raise ValueError(f"normals {normals!r}: None (flat), {' or '.join(map(repr, NORMAL_MODES))} (computed), or a [V,3] array")
            from .mesh import vertex_normals
            self.normals = vertex_normals(self.verts, self.tris.int(), weight=normals, orient='outward')
        else:
            self.normals = None if normals is None else as_t(normals, torch.float32).reshape(V, 3)
        if isinstance(env, (str, os.PathLike)):
            from .envlight import read_hdr
            env = read_hdr(env)
        self.env = as_t(env, torch.float32)
        assert self.env.ndim == 3 and self.env.shape[2] == 3, self.env.shape
        if convention not in CONVENTIONS:
            raise ValueError(f'convention {convention!r}: one of {sorted(CONVENTIONS)}')
        if geometry_type not in GEOMETRY_TYPES:
            raise ValueError(f'geometry_type {geometry_type!r}: one of {sorted(GEOMETRY_TYPES)}')
        self.convention, self.geometry_type = CONVENTIONS[convention], GEOMETRY_TYPES[geometry_type]
        self.rot = None if env_rotation is None else np.asarray(
            env_rotation.detach().cpu().numpy() if torch.is_tensor(env_rotation) else env_rotation, np.float32).reshape(3, 3)
        self.tracer = tracer if tracer is not None else RayTracer(self.verts, self.tris.int(), build=build)
        self._tabs = {}
        self._light = {}
        if bounces not in (0, 1):
            raise ValueError(f'bounces {bounces!r}: 0 (direct lighting) or 1 (one inter-reflection)')
        self.bounces = bounces                                          # what render() takes when it is not told

    @classmethod
    def from_asset(cls, obj_path, env, **kw):
        """the textured asset write_textured_obj stored -- <name>.obj with its MTL and the three maps beside it -- under `env`; **kw: the
        other arguments of Relighter.  When the MTL names a normal map it is passed on as normal_map (normal_map=None in kw: ignore it),
        and `normals` then defaults to the frame mode the asset records ('angle' / 'area'; an asset baked with the caller's own normals
        needs them again)"""
        from .texture import read_textured_obj
        asset = read_textured_obj(obj_path)
        missing = [k for k in ('albedo', 'metallic', 'roughness') if k not in asset]
        if missing:
            raise ValueError(f'{obj_path}: no {", ".join(missing)} map beside it (the MTL names {asset["map_Kd"]!r})')
        if 'normal' in asset and 'normal_map' not in kw:
            kw['normal_map'] = {'normal': asset['normal'], 'vt': asset['vt'], 'ft': asset['ft'], 'space': asset['normal_space']}
            if asset['normal_frame'] in NORMAL_MODES:
                kw.setdefault('normals', asset['normal_frame'])
            elif asset['normal_space'] == 'tangent' and kw.get('normals') is None:
                raise ValueError(f"{obj_path}: its normal map was baked in the frame of the caller's own normals: pass them as normals=")
        return cls(asset['v'], asset['f'], None, env, textures=asset, **kw)

    def light_table(self, clamp=None):
        """the map's sampling table under this relighter's convention and rotation, one per cap (the cap changes the weights)"""
        key = float(clamp or 0.0)
        if key not in self._light:
            self._light[key] = light_table(self.env, self.convention, self.rot, clamp)
        return self._light[key]

    def _table(self, n):
        if n not in self._tabs:
            self._tabs[n] = sample_table(n, self.device)
        return self._tabs[n]

    def camera_rays(self, pose, K, h, w):
        """pixel centres +0.5, the arithmetic of NeROMaterialRenderer._trace_views -> rays_o, rays_d [h w,3]"""
        dev = self.device
        pose = torch.as_tensor(np.asarray(pose.cpu() if torch.is_tensor(pose) else pose), dtype=torch.float32).to(dev).reshape(1, 3, 4)
        K = torch.as_tensor(np.asarray(K.cpu() if torch.is_tensor(K) else K), dtype=torch.float32).to(dev).reshape(1, 3, 3)
        ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
        coords = torch.stack([xs + 0.5, ys + 0.5, torch.ones_like(xs, dtype=torch.float32)], -1).reshape(1, h * w, 3).float()
        Rm, t = pose[:, :, :3], pose[:, :, 3:]
        rays_d = torch.nn.functional.normalize((coords @ torch.inverse(K).permute(0, 2, 1)) @ Rm, dim=-1)
        rays_o = (-Rm.permute(0, 2, 1) @ t).permute(0, 2, 1).repeat(1, h * w, 1)
        return rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()

    def surface(self, rays_o, rays_d, spread=None):
        """trace and interpolate -> dict: depth [n], hit [n] bool, idx [m] (the hit rays), and for those pts, normal, mat5 (PERCEPTUAL
        roughness) [m,.].  With textures mat5 is fetched from the maps at the hits' UVs: spread is the width of a ray's footprint at unit
        distance, which sets the level of detail (None: level 0); without textures it is not read"""
        depth, face, bary = trace_faces(self.tracer, rays_o, rays_d)
        hit = face >= 0
        idx = torch.nonzero(hit)[:, 0]
        f = self.tris[face[idx].long()]                                                      # [m,3]
        u, v = bary[idx, 0:1], bary[idx, 1:2]
        wts = torch.stack([1.0 - u - v, u, v], 1)                                            # [m,3,1]
        corner = self.verts[f]                                                               # [m,3,3]
        pts = (wts * corner).sum(1)
        if self.textures is not None:
            from . import texfetch
            mat5 = texfetch.fetch_materials(self.textures, self.vt, self.ft, self.face_scale, face[idx], bary[idx], depth[idx], spread, self.lod_bias)
        else:
            mat5 = (wts * self.mat5[f]).sum(1)
        if self.normals is None or self._computed_normals:
            # the flat normal on the side the ray came from: the meshes of extract_mesh.py are wound inwards (the reference's trace() negates the
            # tracer's normals), others outwards -- the side a camera ray meets of a closed mesh is its outside either way
            nrm = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
            nrm = torch.where((nrm * rays_d[idx]).sum(-1, keepdim=True) > 0, -nrm, nrm)
        if self.normals is not None:
            smooth = (wts * self.normals[f]).sum(1)
            if self._computed_normals:                                                       # (a caller's own normals are taken as they are)
                good = torch.isfinite(smooth).all(-1, keepdim=True) & (smooth != 0).any(-1, keepdim=True)
                smooth = torch.where(good, smooth, nrm)
            nrm = smooth
        if self.normal_map is not None:
            from . import transfer
            nrm = transfer.apply_normal_map(self.normal_map, self.nm_vt, self.nm_ft, self.nm_scale, self.nm_tangent, self.nm_sign, face[idx],
                                            bary[idx], depth[idx], nrm, spread, self.lod_bias)
        nrm = torch.nn.functional.normalize(nrm, dim=-1)
        return {'depth': depth, 'hit': hit, 'idx': idx, 'pts': pts, 'normal': nrm, 'mat5': mat5}

    def render(self, pose, K, h, w, samples=(128, 128), ssaa=1, seed=0, chunk=None, clamp=None, background=None, bounces=None, denoise=None):
        """one view -> dict of device tensors [h,w,C]: rgb_lin (linear), rgb (linear_to_srgb, clipped to [0,1]), alpha (coverage), albedo,
        metallic, roughness (perceptual), normal, depth (10 where nothing is hit), and rgba8 uint8 [h,w,4] (straight alpha).  samples = (Dd,
        Ds) directions per pixel, or (Dd, Ds, Dl) with Dl more drawn from the map itself and all three combined by multiple importance
        sampling (same expectation, far less noise under a map with a sun or a lamp in it); ssaa = s renders s h x s w
        and box-filters with premultiplied alpha; chunk: hit pixels per kernel call (any value gives the same bits); clamp: cap on the
        environment's radiance per channel (firefly control; it darkens the picture, the third sample count does not); background: linear rgb [3] or
        [h,w,3] behind the uncovered part of a pixel (None: zeros there, rgb_lin is the straight colour); bounces: 0 = direct lighting
        (None: the relighter's default, 0 unless it was built otherwise), 1 = a blocked direction fetches the light of the surface it meets
         -- rgb_lin then holds both, and indirect_lin [h,w,3] the bounced part alone, through the same filter.
        denoise: None or False = off, the bits of a call without the argument; True, or a dict of nero_amd.denoise.denoise's parameters (iterations, sigma_l,
        normal_pow2, sigma_p, sigma_g), filters three signals at the traced resolution (ssaa h x ssaa w), before the box filter (DESIGN.md
        9.12.3): the diffuse term divided by max(albedo (1 - metallic), 1e-4), filtered and multiplied back, so that the filter sees the
        light and not the surface's colour; the specular term; with bounces the indirect term -- the last two with (roughness, metallic,
        luminance of the albedo, 0) as extra guide channels.  rgb_lin is then the sum of the filtered signals, indirect_lin the filtered
        one, and rgb_lin_raw the unfiltered sum through the same box filter and background.  sigma_p defaults to 0.015 x the diagonal of
        the mesh's bounding box: a constant carried over from the analytic scene the filter was prototyped on, NOT tuned on a real render."""
        bounces = self.bounces if bounces is None else bounces
        dn = None
        if denoise is not None and denoise is not False:
            from . import denoise as DN
            dn = DN.options(denoise, 0.015 * float((self.verts.max(0).values - self.verts.min(0).values).norm()))
        if bounces not in (0, 1):
            raise ValueError(f'bounces {bounces!r}: 0 (direct lighting) or 1 (one inter-reflection)')
        s = int(ssaa)
        assert s >= 1
        H, W = s * h, s * w
        Ks = np.diag([float(s), float(s), 1.0]).astype(np.float32) @ np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float32).reshape(3, 3)
        with torch.no_grad():
            rays_o, rays_d = self.camera_rays(pose, Ks, H, W)
            # (textured: a pixel's width at unit distance at the traced resolution sets the level of detail)
            sf = self.surface(rays_o, rays_d) if self.textures is None else self.surface(rays_o, rays_d, spread=1.0 / float(Ks[0, 0]))
            idx, m = sf['idx'], int(sf['idx'].numel())
            if len(samples) not in (2, 3):
                raise ValueError(f'samples {samples!r}: (Dd, Ds) or (Dd, Ds, Dl)')
            Dd, Ds = int(samples[0]), int(samples[1])
            rgb = torch.zeros(H * W, 3, device=self.device)
            ind = torch.zeros(H * W, 3, device=self.device) if bounces else None
            raw = rgb                                                     # (the unfiltered sum, where a filter replaces rgb below)
            if m > 0:
                rand_d, rand_s = pixel_rotations(idx, seed)
                pt = point_records(sf['pts'], -rays_d[idx], sf['normal'], estimator_materials(sf['mat5']), rand_d, rand_s)
                mis = {} if len(samples) == 2 else dict(tab_l=self._table(int(samples[2])), rand_l=pixel_shifts(idx, seed),
                                                        table=self.light_table(clamp))
                if bounces:
                    mis.update(bounces=1, mesh=(self.verts, self.tris.int(), self.mat5, self.normals), key=pixel_keys(idx, seed))
                got = relight_points(self.tracer, pt, self._table(Dd), self._table(Ds), self.env, self.convention, self.rot, clamp,
                                     self.geometry_type, chunk, **mis)
                rgb[idx] = got[0]
                if bounces:
                    ind[idx] = got[3]
                if dn is not None:
                    raw = rgb
                    rgb, ind = self._denoise(dn, H, W, sf, got, bounces)
            alpha = sf['hit'].float().reshape(H * W, 1)
            full = lambda x: torch.zeros(H * W, x.shape[1], device=self.device).index_copy_(0, idx, x)
            planes = torch.cat([rgb, full(sf['mat5']), full(sf['normal']), (sf['depth'].reshape(-1, 1) * alpha), alpha], -1)    # premultiplied
            planes = planes.reshape(h, s, w, s, planes.shape[1]).mean((1, 3))
            a = planes[..., 12:13]
            straight = planes[..., :12] / torch.clamp(a, min=1e-12)
            straight = torch.where(a > 0, straight, torch.zeros_like(straight))
            rgb_lin = straight[..., 0:3]
            if background is not None:
                bg = torch.as_tensor(np.asarray(background.cpu() if torch.is_tensor(background) else background), dtype=torch.float32).to(self.device)
                rgb_lin = planes[..., 0:3] + (1.0 - a) * bg.expand(h, w, 3)
            srgb = torch.clamp(linear_to_srgb(rgb_lin), 0.0, 1.0)
            rgba8 = torch.round(torch.cat([srgb, a], -1) * 255.0).to(torch.uint8)
            nrm = torch.nn.functional.normalize(straight[..., 8:11], dim=-1)
            depth = torch.where(a > 0, straight[..., 11:12], torch.full_like(a, MISS_DEPTH))
            extra = {}
            if bounces:                                                   # the same box filter and the same straightening as rgb_lin's
                ip = ind.reshape(h, s, w, s, 3).mean((1, 3))
                extra['indirect_lin'] = torch.where(a > 0, ip / torch.clamp(a, min=1e-12), torch.zeros_like(ip))
            if dn is not None:                                            # ... and the same background
                rp = raw.reshape(h, s, w, s, 3).mean((1, 3))
                extra['rgb_lin_raw'] = (torch.where(a > 0, rp / torch.clamp(a, min=1e-12), torch.zeros_like(rp)) if background is None
                                        else rp + (1.0 - a) * bg.expand(h, w, 3))
        return {**extra, 'rgb_lin': rgb_lin, 'rgb': srgb, 'alpha': a, 'albedo': straight[..., 5:8], 'metallic': straight[..., 3:4],
                'roughness': straight[..., 4:5], 'normal': nrm, 'depth': depth, 'rgba8': rgba8}

    def _denoise(self, dn, H, W, sf, got, bounces):
        """render(denoise=...)'s filter at the traced resolution: got = relight_points' (rgb, diffuse, specular[, indirect]) over the hit
        pixels sf['idx'] -> (rgb, indirect | None) [H W,3], the filtered signals and their sum"""
        from . import denoise as DN
        idx = sf['idx']
        full = lambda x: torch.zeros(H * W, x.shape[1], device=self.device).index_copy_(0, idx, x)
        pos, nrm, valid = full(sf['pts']), full(sf['normal']), sf['hit'].reshape(-1)
        metallic, rough, albedo = sf['mat5'][:, 0:1], sf['mat5'][:, 1:2], sf['mat5'][:, 2:5]
        demod = full(torch.clamp(albedo * (1.0 - metallic), min=1e-4))
        lum = (0.2126 * albedo[:, 0:1] + 0.7152 * albedo[:, 1:2]) + 0.0722 * albedo[:, 2:3]
        guide_mat = DN.pack_guides(pos, nrm, valid, full(torch.cat([rough, metallic, lum, torch.zeros_like(lum)], -1)))
        guide = guide_mat[:, :8].contiguous()
        run = lambda g, x: DN.denoise_records(g, DN.pack_signal(x), H, W, dn['iterations'], dn['sigma_l'], dn['normal_pow2'], dn['sigma_p'],
                                              dn['sigma_g'])[:, :3]
        diffuse = run(guide, full(got[1]) / torch.where(valid[:, None], demod, torch.ones_like(demod))) * demod
        rgb = diffuse + run(guide_mat, full(got[2]))
        ind = None
        if bounces:
            ind = run(guide_mat, full(got[3]))
            rgb = rgb + ind
        return rgb, ind

    def render_orbit(self, out_dir, num=360, azimuth=0.0, elevation=30.0, dist=3.0, h=800, w=800, K=None, **kw):
        """the reference's relighting orbit: view k of relighting_poses(num, azimuth, elevation, dist), as Blender sees it over the mesh's own
        frame (poses_in_mesh_frame) -> out_dir/k.png (RGBA).  -> the paths"""
        os.makedirs(out_dir, exist_ok=True)
        K = default_K(h, w) if K is None else K
        paths = []
        for k, pose in enumerate(poses_in_mesh_frame(relighting_poses(num, azimuth, elevation, dist))):
            out = self.render(pose, K, h, w, **kw)
            paths.append(os.path.join(out_dir, f'{k}.png'))
            write_rgba_png(paths[-1], out['rgba8'])
        return paths
