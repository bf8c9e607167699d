"""Baking the Stage-II materials into UV texture maps on the device (libnero_hip.so, nero_uv_* / nero_tex_*), and the textured OBJ.

The reference does this in extract_materials_texture_map.py with xatlas (unwrap), nvdiffrast (rasterise / interpolate in UV space), scipy
(dilation / erosion), sklearn (kd-tree gutter fill) and cv2 (resize, images), copying every 640 k-texel chunk to the host.  Every
step is a kernel of nero_amd/csrc/texture.hip or mesh_atlas.hip here:
  * rasterize_uv / interpolate: coverage in UV space by an exact integer rule, positions interpolated in float64 and compacted by prefix sum;
  * quantize: linear_to_srgb, 8 bits;
  * gutter_regions / fill_gutter: the 32-texel gutter filled from the nearest chart-border texel;
  * downsample2: the 2 x 2 mean of the supersampled maps;
  * bake_materials: all of it around NeROMaterialRenderer.predict_materials, the only host traffic being the count readbacks;
  * chart_atlas: the projection atlas in place of xatlas: charts of faces that look along one signed axis, projected at one
    texel density and shelf-packed; uv_overlap measures what such an atlas (or anyone's) covers twice;
  * simple_atlas: a dependency-free one-chart-per-triangle atlas for when no unwrapper is at hand; any (vt, ft) can be passed instead;
  * ambient_occlusion / ao_bytes / bake_ambient_occlusion: an occlusion map from shadow rays on the mesh tracer's BVH (nero_bvh_ao of
    include/nero_hip_visibility.h; the reference has no counterpart), also as bake_materials(..., ao={...});
  * write_textured_obj / read_textured_obj: the reference's OBJ / MTL layout with lossless PNG maps.
Conventions (include/nero_hip.h): maps are [h, w] row-major, texel (row y, column x) has its centre at u = (x + 0.5) / w, v = (y + 0.5) / h."""
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib as L

_lib = L.lib


def _dev(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _to(x, dtype, dev, cols=None):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    x = x.to(device=dev, dtype=dtype).contiguous()
    if cols is not None and (x.dim() != 2 or x.shape[1] != cols):
        raise ValueError(f'expected an array [n, {cols}], got {tuple(x.shape)}')
    return x


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


# ---- kernels --------------------------------------------------------------------------------------------------------------------------------
def rasterize_uv(vt, ft, h, w, out=None):
    """vt [nvt,2] in [0,1] (u along the columns, v along the rows), ft [nt,3] -> tri_id int32 [h, w] on the device, -1 where uncovered
    (nero_uv_raster: the exact-cover integer rule of include/nero_hip.h; overlapping charts resolve to the lowest triangle index).  `out`:
    an int32 [h, w] tensor to write into.  A size outside [1, 16384] or a face index outside [0, nvt) raises NeroHipError, nothing written."""
    dev = _dev(vt, ft, out)
    vt, ft = _to(vt, torch.float32, dev, 2), _to(ft, torch.int32, dev, 3)
    h, w = int(h), int(w)
    with torch.cuda.device(dev):
        need = int(_lib.nero_uv_raster_workspace_bytes(ft.shape[0]))
        ws = _ws(need, dev)
        if out is None:
            out = torch.empty((max(h, 0), max(w, 0)) if max(h, w) <= 16384 else (0, 0), dtype=torch.int32, device=dev)
        L.check(_lib.nero_uv_raster(L.ptr(vt), vt.shape[0], L.ptr(ft), ft.shape[0], h, w, L.ptr(ws), L.ptr(out), L.stream_ptr()))
    return out


def interpolate(tri_id, vt, ft, attr, fa, cap=None, return_mask=False, out=None):
    """the covered texels of tri_id [h, w] in ascending row-major order: (texel int32 [n], values float32 [n, C]) with values = the attribute
    attr [nv, C], indexed by its own faces fa [nt, 3], interpolated at the texel centre in float64 and rounded once (nero_uv_interp).  One
    readback of the count sizes the outputs; `cap`: allocate for that many texels instead (fewer than covered raises NeroHipError, nothing
    written); `out` = (texel, values) buffers to write into; return_mask: also the coverage as bytes [h, w]."""
    dev = _dev(tri_id)
    h, w = tri_id.shape
    tri_id = _to(tri_id, torch.int32, dev)
    vt, ft, fa = _to(vt, torch.float32, dev, 2), _to(ft, torch.int32, dev, 3), _to(fa, torch.int32, dev, 3)
    attr = _to(attr, torch.float32, dev)
    if attr.dim() != 2 or fa.shape != ft.shape:
        raise ValueError(f'interpolate: attr must be [nv, C] and fa shaped like ft, got {tuple(attr.shape)} and {tuple(fa.shape)} vs {tuple(ft.shape)}')
    Cn = attr.shape[1]
    with torch.cuda.device(dev):
        ws = _ws(_lib.nero_uv_interp_workspace_bytes(h, w), dev)
        mask = torch.empty((h, w), dtype=torch.uint8, device=dev) if return_mask else None
        n_out = torch.zeros(1, dtype=torch.int64, device=dev)
        if out is not None:
            texel, vals = out
            cap = texel.shape[0] if cap is None else int(cap)
        else:
            if cap is None:
                cap = int((tri_id >= 0).sum())                      # the count readback that sizes the outputs
            texel = torch.empty(cap, dtype=torch.int32, device=dev)
            vals = torch.empty((cap, Cn), dtype=torch.float32, device=dev)
        L.check(_lib.nero_uv_interp(L.ptr(tri_id), L.ptr(vt), vt.shape[0], L.ptr(ft), ft.shape[0], L.ptr(attr), attr.shape[0], Cn, L.ptr(fa), h, w,
                                    L.ptr(ws), L.ptr(texel), L.ptr(vals), int(cap), L.ptr(mask), L.ptr(n_out), L.stream_ptr()))
        n = int(n_out)
    res = (texel[:n], vals[:n])
    return res + (mask,) if return_mask else res


def quantize(values, texel, h, w):
    """values float32 [n, C] at the texels texel [n] -> uint8 [h, w, C], zero elsewhere: uint8(linear_to_srgb(clamp(x, 0, 1)) * 255), truncated
    (nero_tex_quantize; extract_materials_texture_map.py:127-133)"""
    dev = _dev(values)
    values, texel = _to(values, torch.float32, dev), _to(texel, torch.int32, dev)
    if values.dim() != 2 or texel.shape != values.shape[:1]:
        raise ValueError(f'quantize: values [n, C] and texel [n] expected, got {tuple(values.shape)} and {tuple(texel.shape)}')
    with torch.cuda.device(dev):
        tex = torch.empty((h, w, values.shape[1]), dtype=torch.uint8, device=dev)
        L.check(_lib.nero_tex_quantize(L.ptr(values), L.ptr(texel), values.shape[0], values.shape[1], int(h), int(w), L.ptr(tex), L.stream_ptr()))
    return tex


def gutter_regions(mask, pad=32, border=3):
    """mask [h, w] (non-zero = covered) -> region uint8 [h, w]: 0 nothing, 1 covered interior, 2 covered and in the search band (within
    city-block distance `border` of an uncovered texel or of the image edge), 3 to be filled (uncovered, within city-block distance `pad` of a
    covered texel) -- binary_dilation(iterations=pad) / binary_erosion(iterations=border) of the reference (:136-141) as two separable passes
    (nero_tex_regions).  pad in [0, 64], border in [1, 16]."""
    dev = _dev(mask)
    mask = _to(mask, torch.uint8, dev)
    h, w = mask.shape
    with torch.cuda.device(dev):
        ws = _ws(_lib.nero_tex_regions_workspace_bytes(h, w), dev)
        region = torch.empty((h, w), dtype=torch.uint8, device=dev)
        L.check(_lib.nero_tex_regions(L.ptr(mask), h, w, int(pad), int(border), L.ptr(ws), L.ptr(region), L.stream_ptr()))
    return region


def fill_gutter(tex, region, pad=32, return_source=False):
    """IN PLACE on tex uint8 [h, w, C] (or [h, w]): every region-3 texel takes the bytes of its nearest region-2 texel (squared Euclidean
    distance in integers, ties to the lowest row-major index), searched within `pad` rows and columns (nero_tex_fill; :143-149).  -> tex, or
    (tex, source int32 [h, w]: the source's row-major index, -1 where nothing was filled)."""
    dev = _dev(tex)
    if not (torch.is_tensor(tex) and tex.is_cuda and tex.dtype == torch.uint8 and tex.is_contiguous() and tex.dim() in (2, 3)):
        raise TypeError('fill_gutter works in place on a contiguous CUDA uint8 tensor [h, w, C] or [h, w]')
    h, w = tex.shape[:2]
    region = _to(region, torch.uint8, dev)
    if region.shape != (h, w):
        raise ValueError(f'fill_gutter: region {tuple(region.shape)} does not match the map {(h, w)}')
    with torch.cuda.device(dev):
        src = torch.empty((h, w), dtype=torch.int32, device=dev) if return_source else None
        L.check(_lib.nero_tex_fill(L.ptr(tex), L.ptr(region), h, w, 1 if tex.dim() == 2 else tex.shape[2], int(pad), L.ptr(src), L.stream_ptr()))
    return (tex, src) if return_source else tex


def downsample2(tex):
    """uint8 [2h, 2w, C] (or [2h, 2w]) -> [h, w, C]: (a + b + c + d + 2) >> 2 per 2 x 2 block (nero_tex_downsample2; cv2.resize INTER_LINEAR at
    an exact factor of two, :157-160)"""
    dev = _dev(tex)
    tex = _to(tex, torch.uint8, dev)
    if tex.dim() not in (2, 3) or tex.shape[0] % 2 or tex.shape[1] % 2 or tex.shape[0] < 2 or tex.shape[1] < 2:
        raise ValueError(f'downsample2 wants [2h, 2w, C] or [2h, 2w], got {tuple(tex.shape)}')
    h, w = tex.shape[0] // 2, tex.shape[1] // 2
    with torch.cuda.device(dev):
        out = torch.empty((h, w) + tuple(tex.shape[2:]), dtype=torch.uint8, device=dev)
        L.check(_lib.nero_tex_downsample2(L.ptr(tex), h, w, 1 if tex.dim() == 2 else tex.shape[2], L.ptr(out), L.stream_ptr()))
    return out


# ---- the chart atlas ------------------------------------------------------------------------------------------------------------------------
def uv_overlap(vt, ft, h, w):
    """the number of texel centres of an h x w map that more than one triangle of (vt, ft) covers, by the coverage rule of rasterize_uv (an
    edge two triangles share never counts twice): nero_uv_overlap_count.  For any atlas, an external unwrapper's too.  One readback of the count."""
    dev = _dev(vt, ft)
    vt, ft = _to(vt, torch.float32, dev, 2), _to(ft, torch.int32, dev, 3)
    h, w = int(h), int(w)
    with torch.cuda.device(dev):
        ws = _ws(_lib.nero_uv_overlap_count_workspace_bytes(ft.shape[0], h, w), dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        L.check(_lib.nero_uv_overlap_count(L.ptr(vt), vt.shape[0], L.ptr(ft), ft.shape[0], h, w, L.ptr(ws), L.ptr(count), L.stream_ptr()))
        return int(count)


def pack_charts(box, scale, size, gutter):
    """the rectangles of the charts at `scale` texels per world unit, shelf-packed into a size x size map: box float [K,4] (min_p, min_q, max_p,
    max_q) -> rects int64 [K,4] = (ox, oy, w, h), or None when they do not fit.  w = ceil(extent_p scale) + 1, h likewise (float64); charts in
    the order (-h, -w, chart), left to right on shelves, `gutter` texels between rectangles and between shelves, gutter // 2 texels at the
    four map edges; a new shelf starts when x + w > size - margin; the last shelf must end at or before size - margin."""
    b = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    K = len(b)
    size, gutter = int(size), int(gutter)
    m = gutter // 2
    with np.errstate(invalid='ignore', over='ignore'):
        wf, hf = np.ceil((b[:, 2] - b[:, 0]) * scale) + 1, np.ceil((b[:, 3] - b[:, 1]) * scale) + 1
    if K and not (np.all(wf <= size) and np.all(hf <= size)):        # (NaN and infinity too)
        return None
    w, h = wf.astype(np.int64), hf.astype(np.int64)
    order = np.lexsort((np.arange(K), -w, -h))
    wo, ho = w[order], h[order]
    P = np.concatenate([[0], np.cumsum(wo + gutter)])                # chart j of a shelf that starts at chart s lies at x = m + P[j] - P[s]
    x, y = np.zeros(K, np.int64), np.zeros(K, np.int64)
    s_, top = 0, m
    while s_ < K:
        e = int(np.searchsorted(P, P[s_] + size - 2 * m + gutter, side='right')) - 1      # the charts s_ .. e - 1 end at or before size - m
        if e == s_:
            return None                                             # wider than the map
        x[s_:e] = m + P[s_:e] - P[s_]
        y[s_:e] = top
        top += int(ho[s_]) + gutter                                 # (the first chart of a shelf is its tallest)
        s_ = e
    if K and top - gutter > size - m:
        return None
    rects = np.zeros((K, 4), np.int64)
    rects[order] = np.stack([x, y, wo, ho], -1)
    return rects


def _min_cell_size(K, gutter):
    size = 1
    while pack_charts(np.zeros((K, 4)), 0.0, size, gutter) is None:
        size += 1
    return size


def choose_scale(box, size, gutter=4, texels_per_unit=None):
    """-> (scale, rects, bisection steps): the texel density of chart_atlas.  texels_per_unit is used as it is (ValueError when it does not
    fit).  Otherwise hi = (size - 2 (gutter // 2) - 1) / the largest extent of a chart (1 when that is 0) is taken when it fits; else 32
    bisection steps between lo = 0 and hi (mid = 0.5 (lo + hi); a mid that fits becomes lo) and the result is lo.  Scale 0 makes every
    rectangle one texel; when even that does not fit, ValueError names the smallest size that holds the cells."""
    b = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    if texels_per_unit is not None:
        scale = float(texels_per_unit)
        if not (np.isfinite(scale) and scale >= 0):
            raise ValueError(f'chart_atlas: texels_per_unit must be finite and >= 0, got {texels_per_unit}')
        rects = pack_charts(b, scale, size, gutter)
        if rects is None:
            raise ValueError(f'chart_atlas: {len(b)} charts at {scale} texels per unit do not fit a map of {size} texels with gutter {gutter}')
        return scale, rects, 0
    ext = float(max((b[:, 2] - b[:, 0]).max(), (b[:, 3] - b[:, 1]).max())) if len(b) else 0.0
    if not np.isfinite(ext):
        raise ValueError('chart_atlas: a chart has a box that is not finite')
    hi = max(0.0, (size - 2 * (gutter // 2) - 1) / ext) if ext > 0 else 1.0
    rects = pack_charts(b, hi, size, gutter)
    if rects is not None:
        return hi, rects, 0
    if pack_charts(b, 0.0, size, gutter) is None:
        raise ValueError(f'chart_atlas: {len(b)} charts of one texel each do not fit a map of {size} texels with gutter {gutter}: the smallest '
                         f'size that works is {_min_cell_size(len(b), gutter)}')
    lo, steps = 0.0, 0
    for _ in range(32):
        mid = 0.5 * (lo + hi)
        steps += 1
        if pack_charts(b, mid, size, gutter) is not None:
            lo = mid
        else:
            hi = mid
    return lo, pack_charts(b, lo, size, gutter), steps


class AtlasInfo:
    """what chart_atlas made: n_charts, scale (texels per world unit), rects int64 [K,4] (ox, oy, w, h in texels, host), fill (the area of the
    rectangles over size^2), overlap_texels (texel centres at `size` that more than one triangle covers: 0 unless a chart folds over itself
    in its projection), bisection_steps, charts (nero_amd.mesh.ChartInfo); and on the device chart int32 [T] (-1: no chart), face_class
    int32 [T], nbr int32 [T,3], vt_vertex int32 [n_vt] (the mesh vertex of each UV vertex, xatlas's vmapping; -1 for the last one when a
    face has no chart), vt_chart int32 [n_vt]"""
    __slots__ = ('n_charts', 'scale', 'rects', 'fill', 'overlap_texels', 'bisection_steps', 'charts', 'chart', 'face_class', 'nbr', 'vt_vertex',
                 'vt_chart', 'size', 'gutter')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def chart_corners_device(tris, n_verts, chart, K):
    """tris CUDA int32 [T,3], chart CUDA int32 [T] (face_charts_device) -> (ft int32 [T,3], vt_vertex int32 [n_vt], vt_chart int32 [n_vt]):
    one UV vertex per (chart, mesh vertex) pair in ascending order, plus a last one (-1, -1) for the corners of chartless faces
    (nero_mesh_chart_corners_count / _emit).  One readback of the totals sizes the outputs."""
    dev = tris.device
    T = tris.shape[0]
    need = int(_lib.nero_mesh_chart_corners_workspace_bytes(T))
    if T and need == 0:
        raise L.NeroHipError(f'chart_corners_device: {T} triangles: no workspace ({L.lib.nero_last_error().decode()})')
    L.check_workspace_fits(need + 12 * T, dev, what='chart-corner workspace')
    with torch.cuda.device(dev):
        s = L.stream_ptr()
        ws = _ws(need, dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(_lib.nero_mesh_chart_corners_count(L.ptr(tris) if T else None, T, int(n_verts), L.ptr(chart) if T else None, int(K), L.ptr(ws),
                                                   L.ptr(totals), s))
        n_vt = int(totals[0])
        ft = torch.empty((T, 3), dtype=torch.int32, device=dev)
        vv = torch.empty(n_vt, dtype=torch.int32, device=dev)
        vc = torch.empty(n_vt, dtype=torch.int32, device=dev)
        L.check(_lib.nero_mesh_chart_corners_emit(T, L.ptr(ws), L.ptr(ft) if T else None, L.ptr(vv) if n_vt else None, L.ptr(vc) if n_vt else None,
                                                  n_vt, s))
    return ft, vv, vc


def chart_uv_device(verts, vt_vertex, vt_chart, chart_class, box, rects, scale, size):
    """the UV coordinates of the UV vertices for packed rectangles rects [K,4] (host) at `scale`: float32 [n_vt, 2] (nero_mesh_chart_uv)"""
    dev = verts.device
    n_vt, K = vt_vertex.shape[0], chart_class.shape[0]
    with torch.cuda.device(dev):
        origin = torch.from_numpy(np.ascontiguousarray(np.asarray(rects).reshape(-1, 4)[:, :2], dtype=np.int32)).to(dev)
        vt = torch.empty((n_vt, 2), dtype=torch.float32, device=dev)
        p = lambda x: L.ptr(x) if x.numel() else None
        L.check(_lib.nero_mesh_chart_uv(p(verts), verts.shape[0], p(vt_vertex), p(vt_chart), n_vt, p(chart_class), p(box), p(origin), K, float(scale),
                                        int(size), p(vt), L.stream_ptr()))
    return vt


def chart_atlas(verts, tris, size, gutter=4, texels_per_unit=None):
    """The projection atlas of a mesh: -> (vt float32 [n_vt, 2], ft int32 [T, 3], AtlasInfo), vt and ft on the device, as bake_materials and
    write_textured_obj take them.

    Charts are edge-connected sets of faces whose normals share a dominant signed axis (nero_amd.mesh.face_charts_device); each chart is
    projected along that axis at ONE world-to-texel scale for the whole mesh, so texel density is uniform up to the projection (a factor of
    at most sqrt(3) in length); vertices are duplicated only along the seams between charts.  The chart rectangles are shelf-packed on the
    host (pack_charts), `gutter` texels apart and gutter // 2 from the map edges; the scale is texels_per_unit, or the largest the packing
    admits (choose_scale).  With U = ox + 0.5 + (x_p - min_p) scale a chart covers only texel centres of its own rectangle, at `size` and
    at 2 * size, so charts stay `gutter` texels apart.  Faces with a repeated or out-of-range index, a zero or non-finite
    normal have no chart: their corners share one UV vertex at (0, 0) and the raster covers nothing for them.  Not built: chart merging,
    LSCM-style flattening, rotation when packing.  Same-class faces joined edge by edge can still overlap in projection (a helical ramp
    does; scanned objects ordinarily do not): info.overlap_texels measures it.  Deterministic: the same mesh gives the same atlas bit for
    bit.  Raises ValueError when texels_per_unit does not fit or when the map cannot hold one texel per chart."""
    from . import mesh as M
    dev = _dev(verts, tris)
    size, gutter = int(size), int(gutter)
    if not 1 <= size <= 16384 or gutter < 0:
        raise ValueError(f'chart_atlas: size must be in [1, 16384] and gutter >= 0, got {size} and {gutter}')
    v_d, f_d = _to(verts, torch.float32, dev, 3), _to(tris, torch.int32, dev, 3)
    chart, cls, nbr, ci = M.face_charts_device(v_d, f_d)
    ft, vv, vc = chart_corners_device(f_d, v_d.shape[0], chart, ci.K)
    box = ci.box.cpu().numpy()                                       # K rows: the packing is host work
    scale, rects, steps = choose_scale(box, size, gutter, texels_per_unit)
    vt = chart_uv_device(v_d, vv, vc, ci.chart_class, ci.box, rects, scale, size)
    info = AtlasInfo(n_charts=ci.K, scale=scale, rects=rects, fill=float((rects[:, 2] * rects[:, 3]).sum()) / float(size * size),
                     overlap_texels=uv_overlap(vt, ft, size, size), bisection_steps=steps, charts=ci, chart=chart, face_class=cls, nbr=nbr,
                     vt_vertex=vv, vt_chart=vc, size=size, gutter=gutter)
    return vt, ft, info


# ---- the built-in atlas ---------------------------------------------------------------------------------------------------------------------
def simple_atlas(verts, tris, size):
    """A deterministic atlas with one chart per triangle and no dependencies: -> (vt float32 [3T, 2], ft int32 [T, 3]).

    A FALLBACK, not xatlas: every triangle becomes a right-angled chart of its own, so texture space is used poorly, texel density follows
    nothing, and every edge is a seam.  A full-resolution marching-cubes mesh needs decimation first or a real unwrapper (pass its vt / ft to
    bake_materials): nero_amd.mesh.simplify_mesh_device(target_faces=N) is that decimation (N = 2 (size // 4)^2 triangles fit at `size`).  Layout: G = ceil(sqrt(ceil(T / 2))) cells per side, each s = size // G texels wide, origins on texel corners; triangles 2k
    and 2k + 1 share cell k (row-major), one in the low corner, one in the high corner.  With n = s - 1 the first chart covers the texels
    i + j <= p of the cell and the second those with i + j >= p + 3, i, j <= n - 1 (p = (2n - 5) // 2); the last row and column of a cell stay
    empty.  So at `size` every chart covers at least one texel centre, and texels of two different charts are never 8-neighbours: at least
    one uncovered texel lies between any two charts (two texel steps apart), at `size` and at any multiple of it.  All chart corners are
    quarter texels, exact in float32.  Raises ValueError when the cells would be smaller than 4 texels, naming the smallest size that works."""
    T = int(np.asarray(tris).shape[0])
    size = int(size)
    G = max(1, int(np.ceil(np.sqrt(np.ceil(T / 2)))))
    while G * G * 2 < T:                                            # (float sqrt rounding)
        G += 1
    s = size // G
    if s < 4:
        raise ValueError(f'simple_atlas: {T} triangles need {G} x {G} cells; at size {size} a cell is {s} texels wide, below the minimum of 4: '
                         f'the smallest size that works is {4 * G}')
    n = s - 1
    p = (2 * n - 5) // 2
    q = p + 3
    lo = np.array([[0.25, 0.25], [p + 1.25, 0.25], [0.25, p + 1.25]])
    hi = np.array([[n - 0.25, n - 0.25], [q - n + 0.75, n - 0.25], [n - 0.25, q - n + 0.75]])
    t = np.arange(T)
    cell = t // 2
    origin = np.stack([(cell % G) * s, (cell // G) * s], -1).astype(np.float64)          # (x, y) texels
    local = np.where((t % 2 == 0)[:, None, None], lo[None], hi[None])                     # [T, 3, 2]
    vt = ((origin[:, None, :] + local) / size).reshape(-1, 2).astype(np.float32)
    ft = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    return vt, ft


# ---- ambient occlusion ----------------------------------------------------------------------------------------------------------------------
AO_MAX_RAYS = (1 << 31) - 64            # n * S of one nero_bvh_ao call
AO_MISS = 10.0                          # the tracer's miss distance: the radius of an unbounded query


def ambient_occlusion(tracer, pts, nrm, key, samples=64, radius=None, bias=1e-4, seed=0, chunk=None):
    """how many of `samples` cosine-distributed shadow rays leaving pts [n,3] (lifted by `bias` along the UNIT normals nrm [n,3]) meet the
    mesh of `tracer` (nero_amd.raytracing.RayTracer) within `radius` (None: 10, the tracer's miss distance): int32 counts [n] on the device,
    through nero_bvh_ao -- the rays are made and cast in one kernel and never stored.  key int32 [n] names each point's sample set (the
    texel's row-major index: the result does not depend on the order or the chunking of the points); samples: a power of two in
    [8, 1024].  `chunk` points per call, at most (2^31 - 64) // samples (the default)."""
    dev = _dev(pts, nrm, key)
    pts, nrm, key = _to(pts, torch.float32, dev, 3), _to(nrm, torch.float32, dev, 3), _to(key, torch.int32, dev)
    n, S = pts.shape[0], int(samples)
    if nrm.shape[0] != n or key.shape != (n,):
        raise ValueError(f'ambient_occlusion: pts [n,3], nrm [n,3] and key [n] expected, got {tuple(pts.shape)}, {tuple(nrm.shape)}, {tuple(key.shape)}')
    if S < 8 or S > 1024 or S & (S - 1):
        raise ValueError(f'ambient_occlusion: samples must be a power of two in [8, 1024], got {samples}')
    tmax = AO_MISS if radius is None else float(radius)
    limit = AO_MAX_RAYS // S
    chunk = limit if chunk is None else min(max(1, int(chunk)), limit)
    with torch.cuda.device(dev):
        count = torch.empty(n, dtype=torch.int32, device=dev)
        h, s = tracer._handle(), L.stream_ptr()
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            L.check(_lib.nero_bvh_ao(h, L.ptr(pts[i:i + m]), L.ptr(nrm[i:i + m]), L.ptr(key[i:i + m]), m, S, int(seed) & 0xffffffff, float(bias),
                                     tmax, L.ptr(count[i:i + m]), s))
    return count


def ao_bytes(count, samples):
    """occluded-ray counts of `samples` rays -> the 8-bit ambient-occlusion level, LINEAR (no sRGB curve: nero_tex_quantize is not used):
    floor(255 (S - c) / S + 1 / 2) as (510 (S - c) + S) // (2 S) in integers.  255: nothing in the way; 0: every ray blocked."""
    S = int(samples)
    c = count.to(torch.int64)
    return torch.div(510 * (S - c) + S, 2 * S, rounding_mode='floor').to(torch.uint8)


def face_normals(verts, tris, flip=False):
    """unit geometric normals of the triangles, float32 [T,3] on the device: normalize(cross(v1 - v0, v2 - v0)), negated when `flip` (a mesh
    wound inward, as the renderer's: NeROMaterialRenderer.trace negates the tracer's face normal)"""
    dev = _dev(verts, tris)
    v, f = _to(verts, torch.float32, dev, 3), _to(tris, torch.int32, dev, 3).long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = torch.nn.functional.normalize(torch.linalg.cross(b - a, c - a), dim=-1)
    return -n if flip else n


def _ao_texture(tracer, tri_id, texel, pts, v_d, f_d, flip_normals, samples, radius, bias, seed):
    """the AO pass over the covered texels of a rasterised atlas -> (counts int32 [n], normals [n,3], texture uint8 [H, W, 1], zero elsewhere)"""
    H, W = tri_id.shape
    nrm = face_normals(v_d, f_d, flip_normals)[tri_id.reshape(-1)[texel.long()].long()].contiguous()
    count = ambient_occlusion(tracer, pts, nrm, texel, samples, radius, bias, seed)
    tex = torch.zeros((H, W, 1), dtype=torch.uint8, device=tri_id.device)
    tex.view(-1)[texel.long()] = ao_bytes(count, samples)
    return count, nrm, tex


def bake_ambient_occlusion(verts, tris, vt=None, ft=None, size=1024, ssaa=2, pad=32, border=3, samples=64, radius=None, bias=1e-4, seed=0,
                           flip_normals=False, tracer=None, atlas='triangles', return_intermediates=False):
    """an ambient-occlusion map of a mesh, no network needed -> {'ao' [size, size] uint8 on the device (255: open, 0: shut in), 'mask' [size,
    size] bool, 'vt', 'ft'}.

    Rasterise and interpolate as bake_materials does; at every covered texel cast `samples` cosine-distributed shadow rays from the surface
    point, lifted by `bias` along the geometric normal of the texel's triangle (negated with flip_normals: a mesh wound inward), no further
    than `radius` (None: unbounded); ao_bytes of the counts; gutter fill and 2 x 2 mean as for the material maps.  tracer: a RayTracer of
    the same mesh (one is built when None).  atlas / vt / ft as in bake_materials.  return_intermediates: also 'tri_id', 'texel', 'points',
    'normals', 'ao_count', 'region' and 'texture' (the filled map [H, W, 1]) at the supersampled size."""
    if ssaa not in (1, 2):
        raise ValueError(f'bake_ambient_occlusion: ssaa must be 1 or 2, got {ssaa}')
    if (vt is None) != (ft is None):
        raise ValueError('bake_ambient_occlusion: pass both vt and ft, or neither')
    if atlas not in ('triangles', 'charts'):
        raise ValueError(f"bake_ambient_occlusion: atlas must be 'triangles' or 'charts', got {atlas!r}")
    dev = _dev(verts, tris, vt, ft)
    atlas_info = None
    with torch.cuda.device(dev), torch.no_grad():
        v_d, f_d = _to(verts, torch.float32, dev, 3), _to(tris, torch.int32, dev, 3)
        if vt is None and atlas == 'charts':
            vt, ft, atlas_info = chart_atlas(v_d, f_d, size)
        elif vt is None:
            vt, ft = simple_atlas(_np(verts), _np(tris), size)
        vt_d, ft_d = _to(vt, torch.float32, dev, 2), _to(ft, torch.int32, dev, 3)
        if ft_d.shape[0] != f_d.shape[0]:
            raise ValueError(f'bake_ambient_occlusion: ft has {ft_d.shape[0]} faces, the mesh {f_d.shape[0]}')
        if tracer is None:
            from .raytracing import RayTracer
            tracer = RayTracer(_np(verts), _np(tris))
        H = W = int(size) * ssaa
        tri_id = rasterize_uv(vt_d, ft_d, H, W)
        texel, pts, mask = interpolate(tri_id, vt_d, ft_d, v_d, f_d, return_mask=True)
        count, nrm, tex = _ao_texture(tracer, tri_id, texel, pts, v_d, f_d, flip_normals, samples, radius, bias, seed)
        region = gutter_regions(mask, pad, border)
        tex_ss = fill_gutter(tex, region, pad)
        if ssaa == 2:
            tex = downsample2(tex_ss)
            mask_out = mask.view(size, 2, size, 2).amax(dim=(1, 3)) > 0
        else:
            tex, mask_out = tex_ss, mask > 0
        out = {'ao': tex[..., 0].contiguous(), 'mask': mask_out, 'vt': vt, 'ft': ft}
        if atlas_info is not None:
            out['atlas_info'] = atlas_info
        if return_intermediates:
            out.update(tri_id=tri_id, texel=texel, points=pts, normals=nrm, ao_count=count, region=region, texture=tex_ss)
    return out


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------
def bake_materials(renderer, vt=None, ft=None, size=1024, ssaa=2, pad=32, chunk=1 << 19, border=3, return_intermediates=False, atlas='triangles',
                   ao=None):
    """NeROMaterialRenderer -> {'albedo' [size, size, 3], 'metallic' [size, size], 'roughness' [size, size]: uint8 device tensors, 'mask'
    [size, size] bool (a chart covers the texel), 'vt', 'ft'}: extract_materials_texture_map.py:89-160 on the device.

    Rasterise the UV triangles at size * ssaa, interpolate the mesh vertices at the covered texels, evaluate predict_materials there in chunks
    of `chunk` rows with the packed kernels cached (as predict_materials_of_vertices does), quantise, fill the `pad`-texel gutter at the
    supersampled size, halve.  Channels follow predict_materials_n2m (network/field.py:925-932): albedo, metallic, roughness -- the network's
    roughness WITHOUT the square root predict_materials_of_vertices applies.  Without vt / ft the atlas is made here: atlas='triangles' (the
    default) is simple_atlas of the renderer's mesh at `size`, atlas='charts' is chart_atlas at `size` (the result then also holds
    'atlas_info'); or pass an unwrapper's vt / ft (xatlas).  The only host traffic is the count readbacks of rasterize_uv / interpolate.  The MLPs run
    on this project's fp32-grade engine (the reference: fp16 autocast), so single 8-bit levels can differ from the reference's maps.
    return_intermediates: also 'tri_id', 'texel', 'points', 'values' [n, 5], 'region', 'source' and 'texture' (the filled maps [H, W, 5])
    at the supersampled size.  ao: None, or a dict with any of 'samples' (64), 'radius' (None), 'bias' (1e-4), 'seed' (0): the same
    rasterisation also feeds an ambient-occlusion pass on renderer.ray_tracer (bake_ambient_occlusion with flip_normals=True: the renderer's
    mesh is wound inward), and the result holds 'ao' [size, size] (with return_intermediates 'ao_count' too).  ao=None: nothing changes."""
    if ssaa not in (1, 2):
        raise ValueError(f'bake_materials: ssaa must be 1 or 2, got {ssaa}')
    if ao is not None and (not isinstance(ao, dict) or set(ao) - {'samples', 'radius', 'bias', 'seed'}):
        raise ValueError(f"bake_materials: ao must be None or a dict of 'samples' / 'radius' / 'bias' / 'seed', got {ao!r}")
    verts, tris = renderer.mesh_vertices, renderer.mesh_triangles
    dev = next(renderer.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError('bake_materials runs on the GPU: move the renderer to a CUDA device first')
    if (vt is None) != (ft is None):
        raise ValueError('bake_materials: pass both vt and ft, or neither')
    if atlas not in ('triangles', 'charts'):
        raise ValueError(f"bake_materials: atlas must be 'triangles' or 'charts', got {atlas!r}")
    atlas_info = None
    if vt is None and atlas == 'charts':
        with torch.cuda.device(dev):
            vt, ft, atlas_info = chart_atlas(_to(verts, torch.float32, dev, 3), _to(tris, torch.int32, dev, 3), size)
    elif vt is None:
        vt, ft = simple_atlas(verts, tris, size)
    if np.asarray(ft.cpu() if torch.is_tensor(ft) else ft).shape[0] != tris.shape[0]:
        raise ValueError(f'bake_materials: ft has {len(ft)} faces, the mesh {tris.shape[0]}')
    H = W = int(size) * ssaa
    chunk = max(1, int(chunk))
    with torch.cuda.device(dev), torch.no_grad():
        vt_d, ft_d = _to(vt, torch.float32, dev, 2), _to(ft, torch.int32, dev, 3)
        v_d, f_d = _to(verts, torch.float32, dev, 3), _to(tris, torch.int32, dev, 3)
        tri_id = rasterize_uv(vt_d, ft_d, H, W)
        texel, pts, mask = interpolate(tri_id, vt_d, ft_d, v_d, f_d, return_mask=True)
        n = pts.shape[0]
        values = torch.empty((n, 5), dtype=torch.float32, device=dev)
        kern = renderer._kernels()
        for i in range(0, n, chunk):
            m, r, a = renderer.predict_materials(pts[i:i + chunk], kern)
            values[i:i + chunk, 0:3] = a
            values[i:i + chunk, 3:4] = m
            values[i:i + chunk, 4:5] = r
        tex = quantize(values, texel, H, W)
        region = gutter_regions(mask, pad, border)
        tex, src = fill_gutter(tex, region, pad, return_source=True) if return_intermediates else (fill_gutter(tex, region, pad), None)
        tex_ss = tex
        if ssaa == 2:
            tex = downsample2(tex)
            mask_out = mask.view(size, 2, size, 2).amax(dim=(1, 3)) > 0
        else:
            mask_out = mask > 0
        out = {'albedo': tex[..., 0:3].contiguous(), 'metallic': tex[..., 3].contiguous(), 'roughness': tex[..., 4].contiguous(), 'mask': mask_out,
               'vt': vt, 'ft': ft}
        if atlas_info is not None:
            out['atlas_info'] = atlas_info
        if return_intermediates:
            out.update(tri_id=tri_id, texel=texel, points=pts, values=values, region=region, source=src, texture=tex_ss)
        if ao is not None:
            count, _, ao_tex = _ao_texture(renderer.ray_tracer, tri_id, texel, pts, v_d, f_d, True, ao.get('samples', 64), ao.get('radius'),
                                           ao.get('bias', 1e-4), ao.get('seed', 0))
            ao_tex = fill_gutter(ao_tex, region, pad)
            out['ao'] = (downsample2(ao_tex) if ssaa == 2 else ao_tex)[..., 0].contiguous()
            if return_intermediates:
                out['ao_count'] = count
    return out


# ---- OBJ / MTL / PNG ------------------------------------------------------------------------------------------------------------------------
def _np(x, dtype=None):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x if dtype is None else x.astype(dtype)


def _png_chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def png_bytes(img):
    """uint8 [h, w] (grey) or [h, w, 3] (RGB) -> the bytes of a non-interlaced 8-bit PNG (filter 0 on every row): the writer used where PIL is
    not importable"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError(f'png_bytes: [h, w] or [h, w, 3] expected, got {img.shape}')
    h, w = img.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, -1)], 1)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 0 if img.ndim == 2 else 2, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', ihdr) + _png_chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _png_chunk(b'IEND', b'')


def write_png(path, img, use_pil=None):
    """lossless 8-bit PNG, image row 0 = array row 0 (as cv2.imwrite).  use_pil: None = PIL when importable, else the zlib writer above"""
    img = np.ascontiguousarray(_np(img), dtype=np.uint8)
    if use_pil is None or use_pil:
        try:
            from PIL import Image
            Image.fromarray(img).save(path, format='PNG')
            return
        except ImportError:
            if use_pil:
                raise
    with open(path, 'wb') as fh:
        fh.write(png_bytes(img))


def read_png(path):
    """-> uint8 [h, w] or [h, w, C]: 8-bit grey / RGB / RGBA / grey+alpha non-interlaced PNG, all five row filters (what write_png and PIL
    write), decoded without PIL"""
    data = open(path, 'rb').read()
    if data[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError(f'read_png: {path} is not a PNG')
    at, idat, hdr = 8, [], None
    while at < len(data):
        n, tag = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        at += 12 + n
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat.append(body)
        elif tag == b'IEND':
            break
    w, h, depth, ctype, _, _, interlace = hdr
    ch = {0: 1, 2: 3, 4: 2, 6: 4}.get(ctype)
    if depth != 8 or ch is None or interlace:
        raise ValueError(f'read_png: only 8-bit non-interlaced grey / RGB (with or without alpha) is supported, got depth {depth} type {ctype}')
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), np.uint8).reshape(h, 1 + w * ch)
    out = np.zeros((h, w * ch), np.int32)
    prev = np.zeros(w * ch, np.int32)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:                                                       # filters that look left: sequential per channel
            cur = np.zeros(w * ch, np.int32)
            for i in range(w * ch):
                a = cur[i - ch] if i >= ch else 0
                b = prev[i]
                c = prev[i - ch] if i >= ch else 0
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) >> 1
                elif f == 4:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                else:
                    raise ValueError(f'read_png: unknown row filter {f}')
                cur[i] = (line[i] + pred) & 255
        out[y] = cur
        prev = cur
    out = out.astype(np.uint8)
    return out.reshape(h, w) if ch == 1 else out.reshape(h, w, ch)


def _map_names(name):
    cas = name[5:] if name.startswith('mesh_') and len(name) > 5 else name
    return [f'feat{k}_{cas}.png' for k in range(3)]


def write_textured_obj(dir, verts, tris, vt, ft, maps, name='mesh_0', use_pil=None):
    """the reference's OBJ / MTL layout (extract_materials_texture_map.py:166-197) in `dir`: <name>.obj with `v x y z`, `vt u 1-v`, 1-based
    `f a/b` faces; <name>.mtl whose map_Kd names the albedo image; feat0_<cas>.png (albedo), feat1_<cas>.png (metallic), feat2_<cas>.png
    (roughness), the two scalar maps as three equal channels (COLOR_GRAY2BGR), image row 0 = texel row 0.  maps: the dict bake_materials
    returns.  When it holds 'ao' (bake_materials(..., ao={...})), feat3_<cas>.png (ambient occlusion, three equal channels) is written too
    and the MTL names it in a map_Ka line; without 'ao' the files are what they were.  When it holds 'normal' (nero_amd.transfer.bake_normal_map / bake_asset), feat4_<cas>.png is
    written and the MTL gains `norm feat4_<cas>.png` and the comment `# nero_normal_map space=<tangent|object> normals=<angle|area|custom>`
    (maps['space'], maps['normals']: a tangent-space map means something only with the frame it was baked in); without 'normal' the
    files are byte for byte what they were.  Differences from the reference: lossless PNG instead of
    JPEG.  -> the path of the OBJ."""
    os.makedirs(dir, exist_ok=True)
    v = _np(verts, np.float64).reshape(-1, 3)
    f = _np(tris, np.int64).reshape(-1, 3)
    uv = _np(vt).reshape(-1, 2)
    fuv = _np(ft, np.int64).reshape(-1, 3)
    if f.shape != fuv.shape:
        raise ValueError(f'write_textured_obj: {len(f)} faces but {len(fuv)} UV faces')
    if f.size and (f.min() < 0 or f.max() >= len(v) or fuv.min() < 0 or fuv.max() >= len(uv)):
        raise ValueError('write_textured_obj: a face index is out of range')
    names = _map_names(name)
    keys = ('albedo', 'metallic', 'roughness')
    if 'ao' in maps:
        names, keys = names + [names[0].replace('feat0_', 'feat3_', 1)], keys + ('ao',)
    norm_name = None
    if 'normal' in maps:
        space, frame = maps.get('space', 'tangent'), maps.get('normals', 'angle')
        if space not in ('tangent', 'object') or frame not in ('angle', 'area', 'custom'):
            raise ValueError(f"write_textured_obj: a normal map of space {space!r} and frame normals {frame!r}")
        norm_name = names[0].replace('feat0_', 'feat4_', 1)
        names, keys = names + [norm_name], keys + ('normal',)
    for fname, key in zip(names, keys):
        img = np.ascontiguousarray(_np(maps[key]), dtype=np.uint8)
        if img.ndim == 2:
            img = np.repeat(img[..., None], 3, -1)
        write_png(os.path.join(dir, fname), img, use_pil)
    uv_out = np.stack([uv[:, 0].astype(np.float64), 1.0 - uv[:, 1].astype(np.float64)], -1)
    faces = np.stack([f + 1, fuv + 1], -1).reshape(-1, 6)
    obj = os.path.join(dir, name + '.obj')
    with open(obj, 'w') as fh:
        fh.write(f'mtllib {name}.mtl\n')
        np.savetxt(fh, v, fmt='v %.9g %.9g %.9g')
        np.savetxt(fh, uv_out, fmt='vt %.17g %.17g')
        fh.write('usemtl defaultMat\n')
        np.savetxt(fh, faces, fmt='f %d/%d %d/%d %d/%d')
    with open(os.path.join(dir, name + '.mtl'), 'w') as fh:
        fh.write(f'newmtl defaultMat\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nTr 1\nillum 1\nNs 0\nmap_Kd {names[0]}\n')
        if 'ao' in maps:
            fh.write(f'map_Ka {names[3]}\n')
        if norm_name is not None:
            fh.write(f'norm {norm_name}\n# nero_normal_map space={space} normals={frame}\n')
    return obj


def read_textured_obj(path, load_maps=True):
    """what write_textured_obj writes -> {'v' float64 [V,3], 'f' int64 [T,3], 'vt' float32 [Vt,2] (the file's 1 - v undone), 'ft' int64 [T,3],
    'mtllib', 'map_Kd', 'map_Ka' (only when the MTL has such a line), and with load_maps 'albedo' [h,w,3], 'metallic' [h,w], 'roughness' [h,w] and, when
    the MTL has a map_Ka line, 'ao' [h,w] uint8 from the PNGs beside it; when the MTL has a `norm` line, 'norm' (the file name),
    'normal_space', 'normal_frame' (from the nero_normal_map comment; 'tangent' and 'angle' without one) and with load_maps 'normal' [h,w,3]}"""
    lines = open(path).read().split('\n')
    pick = lambda key: [ln[len(key):] for ln in lines if ln.startswith(key)]
    v = np.array([x.split() for x in pick('v ')], dtype=np.float64).reshape(-1, 3)
    uv = np.array([x.split() for x in pick('vt ')], dtype=np.float64).reshape(-1, 2)
    fl = pick('f ')
    faces = np.array([x.replace('/', ' ').split() for x in fl], dtype=np.int64).reshape(len(fl), 3, 2) - 1
    out = {'v': v, 'f': np.ascontiguousarray(faces[..., 0]), 'vt': np.stack([uv[:, 0], 1.0 - uv[:, 1]], -1).astype(np.float32),
           'ft': np.ascontiguousarray(faces[..., 1]), 'mtllib': (pick('mtllib ') or [None])[0], 'map_Kd': None}
    out['mtllib'] = out['mtllib'].strip() if out['mtllib'] else None
    d = os.path.dirname(os.path.abspath(path))
    if out['mtllib'] and os.path.exists(os.path.join(d, out['mtllib'])):
        mtl = open(os.path.join(d, out['mtllib'])).read().split('\n')
        kd = [ln.split(None, 1)[1].strip() for ln in mtl if ln.startswith('map_Kd ')]
        out['map_Kd'] = kd[0] if kd else None
        ka = [ln.split(None, 1)[1].strip() for ln in mtl if ln.startswith('map_Ka ')]
        if ka:
            out['map_Ka'] = ka[0]
        nm = [ln.split(None, 1)[1].strip() for ln in mtl if ln.startswith('norm ')]
        if nm:
            out['norm'] = nm[0]
            note = dict(kv.split('=', 1) for ln in mtl if ln.startswith('# nero_normal_map ') for kv in ln.split()[2:] if '=' in kv)
            out['normal_space'], out['normal_frame'] = note.get('space', 'tangent'), note.get('normals', 'angle')
            if load_maps and os.path.exists(os.path.join(d, nm[0])):
                out['normal'] = read_png(os.path.join(d, nm[0]))
    if load_maps and out['map_Kd'] and out['map_Kd'].startswith('feat0_'):
        for k, key in enumerate(('albedo', 'metallic', 'roughness')):
            p = os.path.join(d, f'feat{k}_' + out['map_Kd'][6:])
            if os.path.exists(p):
                img = read_png(p)
                out[key] = img if k == 0 else np.ascontiguousarray(img[..., 0])
    if load_maps and 'map_Ka' in out and os.path.exists(os.path.join(d, out['map_Ka'])):
        img = read_png(os.path.join(d, out['map_Ka']))
        out['ao'] = img if img.ndim == 2 else np.ascontiguousarray(img[..., 0])
    return out
