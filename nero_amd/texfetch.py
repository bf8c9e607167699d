"""Mip-mapped UV material lookup for the relighter (include/nero_hip_texfetch.h, nero_amd/csrc/tex_fetch.hip): the maps
bake_materials writes -- albedo, metallic, roughness as 8-bit images over a UV atlas -- read back at the relighter's hits.

  * TextureSet: the three maps as one 8-byte record per texel, reduced to a mip pyramid (every level bit for bit texture.downsample2 of the
    one below), and the 256-entry table that decodes a byte;
  * face_scale: texels per world unit of every face, what turns a pixel's footprint on the surface into texels;
  * fetch_materials: the fused trilinear fetch, one lane per hit -> mat5 as Relighter carries it;
  * vertex_materials: one level-0 fetch per vertex, the stand-in the bounce kernels read at secondary hits.

THE STORED ENCODING.  nero_tex_quantize writes EVERY channel as uint8(linear_to_srgb(clamp(x, 0, 1)) * 255), metallic and roughness too, and
the roughness channel holds the network's alpha = roughness^2 (bake_materials).  srgb_lut() inverts that curve in float64 on the host;
the perceptual roughness of mat5 is sqrt(lut[byte])."""
import numpy as np
import torch

from . import _lib as L

_lib = L.lib
RECORD_BYTES = 8


def srgb_lut():
    """float32 [256]: lut[b] = the float32 rounding of the float64 inverse of this project's linear_to_srgb at s = b / 255: s 25 / 323 for
    s <= 0.04045, ((200 s + 11) / 211) ** 2.4 otherwise"""
    s = np.arange(256, dtype=np.float64) / 255.0
    return np.where(s <= 0.04045, s * 25.0 / 323.0, ((200.0 * s + 11.0) / 211.0) ** 2.4).astype(np.float32)


def mip_levels(h, w):
    """levels of the pyramid of an h x w map: 1 + min(ctz(h), ctz(w)), at most 15 (nero_tex_mip_levels)"""
    n = int(_lib.nero_tex_mip_levels(int(h), int(w)))
    if n == 0:
        raise ValueError(f'a map of {h} x {w}: both sizes must lie in [1, 16384]')
    return n


def _dev_tensor(x, dtype, dev, shape=None):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    x = x.detach().to(device=dev, dtype=dtype).contiguous()
    if shape is not None:
        x = x.reshape(shape)
    return x


class TextureSet:
    """albedo uint8 [h,w,3], metallic uint8 [h,w], roughness uint8 [h,w] (arrays or tensors; what bake_materials and read_textured_obj
    return) -> the packed pyramid on the device: .pyramid uint8 [nero_tex_mip_bytes(h, w)], .lut float32 [256], .h, .w, .levels;
    level(k) is the view [h >> k, w >> k, 8] of level k (bytes r, g, b, metallic, roughness, 0, 0, 0).  out: a contiguous uint8 device
    tensor of exactly that many bytes, 8-byte aligned, to build the pyramid into."""

    def __init__(self, albedo, metallic, roughness, device=None, out=None):
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        albedo = _dev_tensor(albedo, torch.uint8, dev)
        if albedo.dim() != 3 or albedo.shape[2] != 3:
            raise ValueError(f'TextureSet: albedo [h, w, 3] expected, got {tuple(albedo.shape)}')
        h, w = int(albedo.shape[0]), int(albedo.shape[1])
        metallic, roughness = _dev_tensor(metallic, torch.uint8, dev), _dev_tensor(roughness, torch.uint8, dev)
        if tuple(metallic.shape) != (h, w) or tuple(roughness.shape) != (h, w):
            raise ValueError(f'TextureSet: metallic and roughness [{h}, {w}] expected, got {tuple(metallic.shape)} and {tuple(roughness.shape)}')
        self.device, self.h, self.w = dev, h, w
        self.levels = mip_levels(h, w)
        self.lut = torch.from_numpy(srgb_lut()).to(dev)
        with torch.cuda.device(dev):
            need = int(_lib.nero_tex_mip_bytes(h, w))
            if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == need):
                raise ValueError(f'TextureSet: out must be a contiguous CUDA uint8 tensor of {need} bytes')
            self.pyramid = torch.empty(need, dtype=torch.uint8, device=dev) if out is None else out
            L.check(_lib.nero_tex_pack(L.ptr(albedo), L.ptr(metallic), L.ptr(roughness), h, w, L.ptr(self.pyramid), L.stream_ptr()))
            L.check(_lib.nero_tex_mip_build(L.ptr(self.pyramid), h, w, L.stream_ptr()))

    def level(self, k):
        if not 0 <= k < self.levels:
            raise IndexError(f'level {k} of a pyramid of {self.levels}')
        off = sum((self.h >> j) * (self.w >> j) for j in range(k)) * RECORD_BYTES
        hk, wk = self.h >> k, self.w >> k
        return self.pyramid[off:off + hk * wk * RECORD_BYTES].view(hk, wk, RECORD_BYTES)


def face_scale(verts, tris, vt, ft, h, w):
    """texels per world unit of every face, float32 [T] on the device: sqrt(A_uv / A_world) with the UV edges scaled by (w, h); 0 for a
    degenerate face or one with an index out of range (nero_tex_face_scale)"""
    dev = verts.device if torch.is_tensor(verts) and verts.is_cuda else torch.device('cuda', torch.cuda.current_device())
    verts, vt = _dev_tensor(verts, torch.float32, dev, (-1, 3)), _dev_tensor(vt, torch.float32, dev, (-1, 2))
    tris, ft = _dev_tensor(tris, torch.int32, dev, (-1, 3)), _dev_tensor(ft, torch.int32, dev, (-1, 3))
    if tris.shape != ft.shape:
        raise ValueError(f'face_scale: {tris.shape[0]} faces but {ft.shape[0]} UV faces')
    scale = torch.empty(tris.shape[0], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(_lib.nero_tex_face_scale(L.ptr(verts), verts.shape[0], L.ptr(tris), L.ptr(vt), vt.shape[0], L.ptr(ft), tris.shape[0], int(h), int(w),
                                         L.ptr(scale), L.stream_ptr()))
    return scale


def fetch_materials(tex, vt, ft, scale, face, bary, depth, spread=None, lod_bias=0.0, return_debug=False):
    """the fused fetch (nero_tex_materials) at n hits: face [n] int32 (an index into ft; outside [0, T): zeros), bary [n,2], depth [n] ->
    mat5 float32 [n,5] = (metallic, PERCEPTUAL roughness, albedo).  The level of detail follows s = depth * spread * scale[face] *
    2^lod_bias texels under the pixel: spread is the pixel's width at unit distance (None: level 0, a plain bilinear fetch).
    return_debug: also dbg [n,8] = (level, t, x0, y0, fx, fy of that level, u, v), what every lane decided."""
    dev = tex.device
    vt, ft = _dev_tensor(vt, torch.float32, dev, (-1, 2)), _dev_tensor(ft, torch.int32, dev, (-1, 3))
    scale, face = _dev_tensor(scale, torch.float32, dev, (-1,)), _dev_tensor(face, torch.int32, dev, (-1,))
    n = face.shape[0]
    bary, depth = _dev_tensor(bary, torch.float32, dev, (n, 2)), _dev_tensor(depth, torch.float32, dev, (n,))
    if scale.shape[0] != ft.shape[0]:
        raise ValueError(f'fetch_materials: scale holds {scale.shape[0]} faces, ft {ft.shape[0]}')
    mat5 = torch.empty(n, 5, dtype=torch.float32, device=dev)
    dbg = torch.empty(n, 8, dtype=torch.float32, device=dev) if return_debug else None
    with torch.cuda.device(dev):
        L.check(_lib.nero_tex_materials(L.ptr(tex.pyramid), tex.h, tex.w, L.ptr(tex.lut), L.ptr(vt), vt.shape[0], L.ptr(ft), ft.shape[0],
                                        L.ptr(scale), L.ptr(face), L.ptr(bary), L.ptr(depth), n, 0.0 if spread is None else float(spread),
                                        float(np.exp2(np.float64(lod_bias))), L.ptr(mat5), L.ptr(dbg), L.stream_ptr()))
    return (mat5, dbg) if return_debug else mat5


def vertex_materials(tex, vt, tris, ft, n_verts, return_owner=False):
    """mat5 float32 [V,5] per vertex (nero_tex_vertex_materials): the level-0 bilinear fetch at the UV of the vertex's lowest-numbered face
    corner (3 f + c, an integer atomic minimum: the same on every run); zeros for a vertex no face names.  AN APPROXIMATION, for the bounce
    kernels only: they shade the surface met at a secondary hit from per-vertex values, so a bounce sees the maps at the vertex spacing
    (DESIGN.md 9.12.4).  return_owner: also the chosen corner numbers int32 [V] (2^31 - 1: none)."""
    dev = tex.device
    vt, ft = _dev_tensor(vt, torch.float32, dev, (-1, 2)), _dev_tensor(ft, torch.int32, dev, (-1, 3))
    tris = _dev_tensor(tris, torch.int32, dev, (-1, 3))
    if tris.shape != ft.shape:
        raise ValueError(f'vertex_materials: {tris.shape[0]} faces but {ft.shape[0]} UV faces')
    V = int(n_verts)
    owner = torch.empty(V, dtype=torch.int32, device=dev)
    mat5 = torch.empty(V, 5, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(_lib.nero_tex_vertex_materials(L.ptr(tex.pyramid), tex.h, tex.w, L.ptr(tex.lut), L.ptr(vt), vt.shape[0], L.ptr(tris), L.ptr(ft),
                                               tris.shape[0], V, L.ptr(owner), L.ptr(mat5), L.stream_ptr()))
    return (mat5, owner) if return_owner else mat5
