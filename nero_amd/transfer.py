"""Detail transfer from a dense mesh (the source) to a simplified one with a UV atlas (the target), on the device (include/nero_transfer.h,
nero_amd/csrc/detail_transfer.hip).

Simplification throws the fine shape away; a normal map brings its shading back.  Every covered texel of the target's atlas is projected
onto the source with the exact closest-point query (RayTracer.closest), the source's shading normal is interpolated there and written in
the target's tangent frame (or in object space):
  * attributes_at: a per-vertex attribute at the (face, bary) pairs closest / trace_faces return;
  * uv_tangents: per-UV-vertex tangents and per-face handedness, order-free integer sums;
  * bake_normal_map: rasterise, interpolate, project, encode, fill the gutter, halve -- the pipeline of texture.bake_materials;
  * bake_asset: the whole asset of a simplified mesh: the material networks evaluated at the PROJECTED points, and the normal map;
  * NormalMap / apply_normal_map: the 4-byte records, their mip pyramid and the fused lookup Relighter(normal_map=...) calls.
THE FRAME (include/nero_transfer.h): T' is the interpolated tangent made orthogonal to the normal, B = face_sign (n x T') points along
increasing FILE v (green up, the OpenGL convention).  It is NOT MikkTSpace: a tool that rebuilds tangents its own way shades a
tangent-space map slightly differently near seams; an object-space map (space='object') has no such dependence."""
import numpy as np
import torch

from . import _lib as L
from . import texture as TX

_lib = L.lib
RECORD_BYTES = 4
SPACES = {'tangent': 0, 'object': 1}
FLAT = (128, 128, 255)


def _space(space):
    if space not in SPACES:
        raise ValueError(f"space must be 'tangent' or 'object', got {space!r}")
    return SPACES[space]


def _t(x, dtype, dev, shape=None):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    x = x.detach().to(device=dev, dtype=dtype).contiguous()
    return x if shape is None else x.reshape(shape)


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device('cuda', torch.cuda.current_device())


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------------
def attributes_at(attr, tris, face, bary, fill=0.0):
    """attr [V,C] (C in [1, 8]; [V] counts as C = 1) of a mesh with triangles tris [T,3], at face [n] int32 and bary [n,2] = the weights
    (b1, b2) of the face's second and third corner -- what RayTracer.closest and relight.trace_faces return -> float32 [n,C]:
    a0 + (b1 (a1 - a0) + b2 (a2 - a0)) (nero_mesh_attr_at).  A face outside [0, T), or one that names a vertex outside [0, V), gives
    `fill`.  Tensors in, device tensors out; numpy in, numpy out."""
    as_numpy = not any(torch.is_tensor(x) for x in (attr, tris, face, bary))
    dev = _device_of(attr, tris, face, bary)
    attr = _t(attr, torch.float32, dev)
    flat = attr.dim() == 1
    attr = attr.reshape(attr.shape[0], -1)
    tris, face = _t(tris, torch.int32, dev, (-1, 3)), _t(face, torch.int32, dev, (-1,))
    n, Cn = face.shape[0], attr.shape[1]
    bary = _t(bary, torch.float32, dev, (n, 2))
    out = torch.empty((n, Cn), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(_lib.nero_mesh_attr_at(L.ptr(attr), attr.shape[0], Cn, L.ptr(tris), tris.shape[0], L.ptr(face), L.ptr(bary), n, float(fill),
                                       L.ptr(out), L.stream_ptr()))
    out = out[:, 0] if flat else out
    return out.cpu().numpy() if as_numpy else out


def uv_tangents(verts, tris, vt, ft, return_info=False):
    """-> (tangent float32 [Vt,3], face_sign int8 [T][, info int64 [4]]) on the device (nero_uv_tangents): per UV vertex -- a seam keeps a
    frame per side -- the unit tangent along increasing u, the area-weighted sum of its faces' tangents, the same bits on every run and
    for every order of the triangles; per face the handedness of its chart as a file stores it (+1, -1 mirrored, 0 for a face that is
    degenerate in UV or in space or names an index out of range: it contributes nothing).  info = (refused faces, degenerate faces, UV
    vertices written as zero, the exponent of the fixed-point scale)."""
    dev = _device_of(verts, tris, vt, ft)
    verts, vt = _t(verts, torch.float32, dev, (-1, 3)), _t(vt, torch.float32, dev, (-1, 2))
    tris, ft = _t(tris, torch.int32, dev, (-1, 3)), _t(ft, torch.int32, dev, (-1, 3))
    if tris.shape != ft.shape:
        raise ValueError(f'uv_tangents: {tris.shape[0]} faces but {ft.shape[0]} UV faces')
    Vt, T = vt.shape[0], tris.shape[0]
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(_lib.nero_uv_tangents_workspace_bytes(Vt, T)), 256), dtype=torch.uint8, device=dev)
        tangent = torch.zeros((Vt, 3), dtype=torch.float32, device=dev)
        sign = torch.zeros(T, dtype=torch.int8, device=dev)
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        L.check(_lib.nero_uv_tangents(L.ptr(verts), verts.shape[0], L.ptr(tris), L.ptr(vt), Vt, L.ptr(ft), T, L.ptr(ws), L.ptr(tangent),
                                      L.ptr(sign), L.ptr(info), L.stream_ptr()))
    return (tangent, sign, info) if return_info else (tangent, sign)


def encode_normals(nrm, tan, sign, ns, valid, texel, h, w, space='tangent', out=None):
    """the bytes of a normal map at covered texels (nero_nmap_encode): frame normals nrm [n,3], tangents tan [n,3], sign int8 [n] (the
    face_sign of each texel's triangle), source normals ns [n,3], valid [n] (0: no source in reach), texel int32 [n] (row-major) ->
    (map uint8 [h,w,3], zero where no texel was written, or `out` written into; the number of invalid texels, a device int64 scalar)"""
    dev = _device_of(nrm, tan, ns, texel)
    nrm, tan, ns = (_t(x, torch.float32, dev, (-1, 3)) for x in (nrm, tan, ns))
    n = nrm.shape[0]
    sign, valid, texel = _t(sign, torch.int8, dev, (n,)), _t(valid, torch.uint8, dev, (n,)), _t(texel, torch.int32, dev, (n,))
    if tan.shape[0] != n or ns.shape[0] != n:
        raise ValueError(f'encode_normals: {n} frame normals, {tan.shape[0]} tangents, {ns.shape[0]} source normals')
    h, w = int(h), int(w)
    if out is None:
        out = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (h, w, 3)):
        raise ValueError(f'encode_normals: out must be a contiguous CUDA uint8 tensor [{h}, {w}, 3]')
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(_lib.nero_nmap_encode(L.ptr(nrm), L.ptr(tan), L.ptr(sign), L.ptr(ns), L.ptr(valid), L.ptr(texel), n, h, w, _space(space),
                                      L.ptr(out), L.ptr(bad), L.stream_ptr()))
    return out, bad


class NormalMap:
    """normal uint8 [h,w,3] (array or tensor: what bake_normal_map and read_textured_obj return) -> the records (x, y, z, 0) and their mip
    pyramid on the device, every level (a + b + c + d + 2) >> 2 of the one below: .pyramid uint8 [nero_nmap_mip_bytes(h, w)], .h, .w,
    .levels, .space; level(k) is the view [h >> k, w >> k, 4] of level k.  A flat map is flat at every level."""

    def __init__(self, normal, space='tangent', device=None):
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        normal = _t(normal, torch.uint8, dev)
        if normal.dim() != 3 or normal.shape[2] != 3:
            raise ValueError(f'NormalMap: normal [h, w, 3] expected, got {tuple(normal.shape)}')
        self.space, self.space_id = space, _space(space)
        self.device, self.h, self.w = dev, int(normal.shape[0]), int(normal.shape[1])
        from .texfetch import mip_levels
        self.levels = mip_levels(self.h, self.w)
        with torch.cuda.device(dev):
            self.pyramid = torch.empty(int(_lib.nero_nmap_mip_bytes(self.h, self.w)), dtype=torch.uint8, device=dev)
            L.check(_lib.nero_nmap_pack(L.ptr(normal), self.h, self.w, L.ptr(self.pyramid), L.stream_ptr()))
            L.check(_lib.nero_nmap_mip_build(L.ptr(self.pyramid), self.h, self.w, L.stream_ptr()))

    def level(self, k):
        if not 0 <= k < self.levels:
            raise IndexError(f'level {k} of a pyramid of {self.levels}')
        off = sum((self.h >> j) * (self.w >> j) for j in range(k)) * RECORD_BYTES
        hk, wk = self.h >> k, self.w >> k
        return self.pyramid[off:off + hk * wk * RECORD_BYTES].view(hk, wk, RECORD_BYTES)


def apply_normal_map(nmap, vt, ft, scale, tangent, face_sign, face, bary, depth, nrm_in, spread=None, lod_bias=0.0, return_debug=False):
    """the fused lookup (nero_nmap_apply) at n hits: the map is fetched at the hits' UVs with the trilinear filter and the level-of-detail
    rule of texfetch.fetch_materials (scale = texfetch.face_scale; spread None: level 0) and, in tangent space, turned into the frame of
    nrm_in [n,3] (any length), the interpolated `tangent` [Vt,3] and face_sign [T] (uv_tangents) -> float32 [n,3], NOT normalised, of
    nrm_in's length.  Where the result is not finite, zero or faces away from nrm_in, and where face is outside [0, T), nrm_in comes
    back; a texel that decodes to (0, 0, 1) returns nrm_in exactly.  return_debug: also dbg [n,8] = (level, t, x0, y0, fx, fy, u, v)."""
    dev = nmap.device
    vt, ft = _t(vt, torch.float32, dev, (-1, 2)), _t(ft, torch.int32, dev, (-1, 3))
    scale, face = _t(scale, torch.float32, dev, (-1,)), _t(face, torch.int32, dev, (-1,))
    tangent, face_sign = _t(tangent, torch.float32, dev, (-1, 3)), _t(face_sign, torch.int8, dev, (-1,))
    n = face.shape[0]
    bary, depth, nrm_in = _t(bary, torch.float32, dev, (n, 2)), _t(depth, torch.float32, dev, (n,)), _t(nrm_in, torch.float32, dev, (n, 3))
    if scale.shape[0] != ft.shape[0] or face_sign.shape[0] != ft.shape[0] or tangent.shape[0] != vt.shape[0]:
        raise ValueError(f'apply_normal_map: {ft.shape[0]} UV faces, {scale.shape[0]} scales, {face_sign.shape[0]} signs; {vt.shape[0]} UV vertices, '
                         f'{tangent.shape[0]} tangents')
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dbg = torch.empty((n, 8), dtype=torch.float32, device=dev) if return_debug else None
    with torch.cuda.device(dev):
        L.check(_lib.nero_nmap_apply(L.ptr(nmap.pyramid), nmap.h, nmap.w, L.ptr(vt), vt.shape[0], L.ptr(ft), ft.shape[0], L.ptr(scale), L.ptr(tangent),
                                     L.ptr(face_sign), L.ptr(face), L.ptr(bary), L.ptr(depth), L.ptr(nrm_in), n, 0.0 if spread is None else float(spread),
                                     float(np.exp2(np.float64(lod_bias))), nmap.space_id, L.ptr(out), L.ptr(dbg), L.stream_ptr()))
    return (out, dbg) if return_debug else out


# ---- the bake ---------------------------------------------------------------------------------------------------------------------------------
def _source_mesh(source, dev):
    """a RayTracer or a (verts, tris) pair -> (tracer, verts float32 [V,3], tris int32 [T,3] on the device)"""
    from .raytracing import RayTracer
    if isinstance(source, RayTracer):
        v, f = source._device_arrays() if source.build == 'device' else source._host_arrays()
        return source, _t(v, torch.float32, dev, (-1, 3)), _t(f, torch.int32, dev, (-1, 3))
    v, f = source
    v, f = _t(v, torch.float32, dev, (-1, 3)), _t(f, torch.int32, dev, (-1, 3))
    return RayTracer(v, f, build='device'), v, f


def _frame_normals(normals, v_d, f_d):
    from .mesh import vertex_normals
    if isinstance(normals, str):
        if normals not in ('angle', 'area'):
            raise ValueError(f"normals must be 'angle', 'area' or a [V,3] array, got {normals!r}")
        return vertex_normals(v_d, f_d, weight=normals, orient='outward'), normals
    return _t(normals, torch.float32, v_d.device, (v_d.shape[0], 3)), 'custom'


def source_normals_at(src_v, src_f, face, bary, mode='angle'):
    """the source's shading normal at (face, bary): 'angle' / 'area' interpolates vertex_normals(orient='outward'), 'face' takes the hit
    face's own unit normal, oriented like them; zeros where face is -1"""
    from .mesh import vertex_normals, winding_sign
    if mode == 'face':
        fn = TX.face_normals(src_v, src_f) * float(winding_sign(src_v, src_f))
        ok = (face >= 0) & (face < src_f.shape[0])
        return torch.where(ok[:, None], fn[face.clamp(0, src_f.shape[0] - 1).long()], torch.zeros((), device=fn.device)).contiguous()
    if mode not in ('angle', 'area'):
        raise ValueError(f"source_normals must be 'angle', 'area' or 'face', got {mode!r}")
    return attributes_at(vertex_normals(src_v, src_f, weight=mode, orient='outward'), src_f, face, bary, fill=0.0)


def _atlas(v_d, f_d, vt, ft, size, atlas, who, gutter=4):
    if (vt is None) != (ft is None):
        raise ValueError(f'{who}: pass both vt and ft, or neither')
    if atlas not in ('triangles', 'charts'):
        raise ValueError(f"{who}: atlas must be 'triangles' or 'charts', got {atlas!r}")
    info = None
    if vt is None and atlas == 'charts':
        vt, ft, info = TX.chart_atlas(v_d, f_d, size, gutter=gutter)
    elif vt is None:
        vt, ft = TX.simple_atlas(v_d.cpu().numpy(), f_d.cpu().numpy(), size)
    return vt, ft, info


def _finish(tex, region, pad, ssaa):
    tex = TX.fill_gutter(tex, region, pad)
    return tex, (TX.downsample2(tex) if ssaa == 2 else tex)


def _project(tracer, src_v, src_f, tri_id, vt_d, ft_d, v_d, f_d, nrm_v, max_dist, source_normals):
    """what the normal bake and the asset bake share: the covered texels, their points, frames, the closest query and the source normals"""
    texel, pts, mask = TX.interpolate(tri_id, vt_d, ft_d, v_d, f_d, return_mask=True)
    n = pts.shape[0]
    _, nrm = TX.interpolate(tri_id, vt_d, ft_d, nrm_v, f_d, cap=n)
    tangent, face_sign = uv_tangents(v_d, f_d, vt_d, ft_d)
    _, tan = TX.interpolate(tri_id, vt_d, ft_d, tangent, ft_d, cap=n)
    sign = face_sign[tri_id.reshape(-1)[texel.long()].long()].contiguous()
    dist, face, bary, point = tracer.closest(pts, max_dist)
    ns = source_normals_at(src_v, src_f, face, bary, source_normals)
    return dict(texel=texel, points=pts, mask=mask, frame_normals=nrm, tangents=tan, sign=sign, dist=dist, face=face, bary=bary, closest=point,
                source_normals=ns, tangent=tangent, face_sign=face_sign)


def _moved(dist, face):
    ok = face >= 0
    return float(dist[ok].max()) if bool(ok.any()) else 0.0


def bake_normal_map(verts, tris, source, vt=None, ft=None, size=1024, ssaa=2, pad=32, border=3, space='tangent', normals='angle',
                    source_normals='angle', max_dist=None, atlas='triangles', return_intermediates=False):
    """High-to-low baking: the shading normals of `source` -- a RayTracer over the dense mesh, or a (verts, tris) pair -- written over the
    atlas of the target mesh (verts, tris) -> {'normal' uint8 [size,size,3] on the device, 'mask' [size,size] bool, 'vt', 'ft', 'space',
    'normals', 'unmatched' (int: covered texels with no source within max_dist, or with no usable source normal; they hold the flat
    value), 'max_moved' (the largest closest distance)}, and 'atlas_info' with atlas='charts'.

    Rasterise the UV triangles at size * ssaa; interpolate position, frame normal and tangent at the covered texels; project each point
    onto the source (RayTracer.closest: exact, nearest point, NOT a ray along the normal -- in a deep concave crease the nearest point can
    lie on the opposite wall; max_dist bounds how far a texel may reach); take the source's normal there (source_normals: 'angle' /
    'area' vertex normals stored outward, or 'face'); encode; fill the gutter and halve as bake_materials does.  normals: how the TARGET's
    frame normal is made -- 'angle' | 'area' through vertex_normals(orient='outward'), or a [V,3] array ('custom' in the result) -- and a
    tangent-space map is only meaningful with the same frame at lookup, so the result records it.  vt / ft / atlas as in bake_materials.
    return_intermediates: also 'tri_id', 'texel', 'points', 'frame_normals', 'tangents', 'sign', 'dist', 'face', 'bary', 'closest',
    'source_normals', 'tangent', 'face_sign', 'region' and 'texture' (the map [H, W, 3] before the gutter fill) at the supersampled size."""
    if ssaa not in (1, 2):
        raise ValueError(f'bake_normal_map: ssaa must be 1 or 2, got {ssaa}')
    _space(space)
    dev = _device_of(verts, tris, vt, ft)
    with torch.cuda.device(dev), torch.no_grad():
        v_d, f_d = _t(verts, torch.float32, dev, (-1, 3)), _t(tris, torch.int32, dev, (-1, 3))
        vt, ft, atlas_info = _atlas(v_d, f_d, vt, ft, size, atlas, 'bake_normal_map')
        vt_d, ft_d = _t(vt, torch.float32, dev, (-1, 2)), _t(ft, torch.int32, dev, (-1, 3))
        if ft_d.shape[0] != f_d.shape[0]:
            raise ValueError(f'bake_normal_map: ft has {ft_d.shape[0]} faces, the mesh {f_d.shape[0]}')
        tracer, src_v, src_f = _source_mesh(source, dev)
        nrm_v, mode = _frame_normals(normals, v_d, f_d)
        H = W = int(size) * ssaa
        tri_id = TX.rasterize_uv(vt_d, ft_d, H, W)
        pr = _project(tracer, src_v, src_f, tri_id, vt_d, ft_d, v_d, f_d, nrm_v, max_dist, source_normals)
        tex, bad = encode_normals(pr['frame_normals'], pr['tangents'], pr['sign'], pr['source_normals'], pr['face'] >= 0, pr['texel'], H, W, space)
        raw = tex.clone() if return_intermediates else None
        region = TX.gutter_regions(pr['mask'], pad, border)
        _, out_tex = _finish(tex, region, pad, ssaa)
        mask = pr['mask']
        mask_out = mask.view(size, 2, size, 2).amax(dim=(1, 3)) > 0 if ssaa == 2 else mask > 0
        out = {'normal': out_tex, 'mask': mask_out, 'vt': vt, 'ft': ft, 'space': space, 'normals': mode, 'unmatched': int(bad),
               'max_moved': _moved(pr['dist'], pr['face'])}
        if atlas_info is not None:
            out['atlas_info'] = atlas_info
        if return_intermediates:
            pr.pop('mask')
            out.update(pr, tri_id=tri_id, region=region, texture=raw)
    return out


def bake_asset(renderer, verts=None, tris=None, target_faces=None, vt=None, ft=None, size=1024, ssaa=2, pad=32, border=3, atlas='charts',
               space='tangent', normals='angle', source_normals='angle', max_dist=None, chunk=1 << 19, gutter=4):
    """The whole asset of a SIMPLIFIED mesh: what bake_materials returns -- 'albedo', 'metallic', 'roughness', 'mask', 'vt', 'ft' -- plus
    'normal', 'space', 'normals', 'verts', 'tris' (the target, on the device), 'unmatched' and 'max_moved'.

    The target is (verts, tris), or simplify_mesh_device of the renderer's own mesh to target_faces, or that mesh itself; the source is
    the renderer's mesh through renderer.ray_tracer.  Every covered texel is projected onto the source with the closest-point query and
    renderer.predict_materials is evaluated AT THE PROJECTED POINT (in chunks, the packed kernels cached), so the material networks are
    asked on the surface they were trained on, not up to a cluster cell away from it; the five channels are quantised, filled and halved
    by bake_materials' calls, and the normal map comes from the same rasterisation and the same query.  A texel with no source within
    max_dist keeps its own point.  gutter: texels between the charts of atlas='charts' (chart_atlas).  The source's normals are stored outward, so the renderer's inward winding does not matter.  Not
    built: ambient occlusion on the transferred asset (bake_ambient_occlusion of the target mesh stands in)."""
    if ssaa not in (1, 2):
        raise ValueError(f'bake_asset: ssaa must be 1 or 2, got {ssaa}')
    _space(space)
    dev = next(renderer.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError('bake_asset runs on the GPU: move the renderer to a CUDA device first')
    if (verts is None) != (tris is None):
        raise ValueError('bake_asset: pass both verts and tris, or neither')
    with torch.cuda.device(dev), torch.no_grad():
        src_v, src_f = _t(renderer.mesh_vertices, torch.float32, dev, (-1, 3)), _t(renderer.mesh_triangles, torch.int32, dev, (-1, 3))
        if verts is not None:
            v_d, f_d = _t(verts, torch.float32, dev, (-1, 3)), _t(tris, torch.int32, dev, (-1, 3))
        elif target_faces is not None:
            from .mesh import simplify_mesh_device
            v_d, f_d = simplify_mesh_device(src_v, src_f, target_faces=int(target_faces))[:2]
            v_d, f_d = v_d.contiguous(), f_d.to(torch.int32).contiguous()
        else:
            v_d, f_d = src_v, src_f
        vt, ft, atlas_info = _atlas(v_d, f_d, vt, ft, size, atlas, 'bake_asset', gutter)
        vt_d, ft_d = _t(vt, torch.float32, dev, (-1, 2)), _t(ft, torch.int32, dev, (-1, 3))
        if ft_d.shape[0] != f_d.shape[0]:
            raise ValueError(f'bake_asset: ft has {ft_d.shape[0]} faces, the mesh {f_d.shape[0]}')
        nrm_v, mode = _frame_normals(normals, v_d, f_d)
        H = W = int(size) * ssaa
        tri_id = TX.rasterize_uv(vt_d, ft_d, H, W)
        pr = _project(renderer.ray_tracer, src_v, src_f, tri_id, vt_d, ft_d, v_d, f_d, nrm_v, max_dist, source_normals)
        found = pr['face'] >= 0
        at = torch.where(found[:, None], pr['closest'], pr['points']).contiguous()
        n = at.shape[0]
        values = torch.empty((n, 5), dtype=torch.float32, device=dev)
        kern = renderer._kernels()
        chunk = max(1, int(chunk))
        for i in range(0, n, chunk):
            m, r, a = renderer.predict_materials(at[i:i + chunk], kern)
            values[i:i + chunk, 0:3] = a
            values[i:i + chunk, 3:4] = m
            values[i:i + chunk, 4:5] = r
        region = TX.gutter_regions(pr['mask'], pad, border)
        _, tex = _finish(TX.quantize(values, pr['texel'], H, W), region, pad, ssaa)
        ntex, bad = encode_normals(pr['frame_normals'], pr['tangents'], pr['sign'], pr['source_normals'], found, pr['texel'], H, W, space)
        _, ntex = _finish(ntex, region, pad, ssaa)
        mask = pr['mask']
        mask_out = mask.view(size, 2, size, 2).amax(dim=(1, 3)) > 0 if ssaa == 2 else mask > 0
        out = {'albedo': tex[..., 0:3].contiguous(), 'metallic': tex[..., 3].contiguous(), 'roughness': tex[..., 4].contiguous(), 'mask': mask_out,
               'vt': vt, 'ft': ft, 'normal': ntex, 'space': space, 'normals': mode, 'verts': v_d, 'tris': f_d, 'unmatched': int(bad),
               'max_moved': _moved(pr['dist'], pr['face'])}
        if atlas_info is not None:
            out['atlas_info'] = atlas_info
    return out
