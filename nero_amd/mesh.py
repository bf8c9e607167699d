"""Marching cubes on the device (libnero_hip.so, nero_mcubes_*) and PLY mesh IO: the Stage-I -> Stage-II handoff without third-party packages.

The reference extracts the Stage-I mesh with PyMCubes (`mcubes.marching_cubes`, network/field.py:1110-1117, extract_mesh.py:24-31) and writes /
reads it with trimesh (extract_mesh.py:34-37, network/renderer.py:704).  This module provides both:
  * marching_cubes_device(u, threshold): the HIP kernels on a CUDA grid -> device tensors;
  * marching_cubes(volume, isovalue): PyMCubes' signature on numpy arrays, so `sys.modules['mcubes'] = nero_amd.mesh` runs the reference's own
    extract_geometry / extract_mesh.py unmodified;
  * write_ply / read_ply: the binary PLY the reference's Stage II reads (`cfg['mesh']`);
  * connected_components_device / clean_mesh_device / clean_mesh: the connected components of a mesh, their statistics, and the mesh without
    the unwanted ones (floaters, inner shells, scraps of the support surface), on the device (nero_mesh_*).  The reference has no
    counterpart: its users delete the debris in a mesh editor.
  * simplify_mesh_device / simplify_mesh / simplify_cells: the mesh reduced to one vertex per occupied cell of a uniform grid, placed by the
    cell's quadric (nero_mesh_simplify_*), for the ray tracer and the texture atlas of Stage II.  Deterministic and exactly specified
    ("Mesh simplification").
  * face_adjacency_device / face_charts_device: the neighbours of every face across its edges and the charts of the projection atlas
    (nero_mesh_face_adjacency / nero_mesh_chart_*), which nero_amd.texture.chart_atlas turns into UV coordinates.
  * vertex_normals / winding_sign: smooth per-vertex normals, face normals weighted by angle or by area and summed as integers
    (nero_vertex_normals), and the side a closed mesh's winding points to; write_ply / read_ply carry the normals.
Conventions (include/nero_hip.h): a corner is inside when u < threshold; vertices are index-space, one per crossing grid edge, ordered by
(linear grid index, axis x<y<z); triangles are ordered by (cell, table position) and wound so that their normals point into u < threshold --
inward for an SDF, which NeROMaterialRenderer.trace flips to outward shading normals."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L

_INT31 = 1 << 31


def workspace_bytes(shape):
    """device bytes nero_mcubes_count / _emit need beside the grid (< 6 bytes per grid point + 64 KiB)"""
    nx, ny, nz = (int(s) for s in shape)
    return int(L.lib.nero_mcubes_workspace_bytes(nx, ny, nz))


def marching_cubes_device(u, threshold=0.0):
    """u: CUDA float32 [nx, ny, nz] (x, y, z order, z fastest: NeROShapeRenderer's grid) -> (verts float32 [V,3] in index space,
    tris int32 [T,3]) on u's device.  One readback of the 16-byte totals between the two launches sizes the outputs exactly."""
    if not (torch.is_tensor(u) and u.is_cuda and u.dtype == torch.float32 and u.dim() == 3):
        raise TypeError(f'marching_cubes_device wants a CUDA float32 [nx, ny, nz] tensor, got '
                        f'{tuple(u.shape) if torch.is_tensor(u) else type(u).__name__} {getattr(u, "dtype", "")}')
    u = u.contiguous()
    nx, ny, nz = u.shape
    dev = u.device
    need = workspace_bytes(u.shape)
    if need == 0:
        raise ValueError(f'marching_cubes_device: grid {nx} x {ny} x {nz} is not supported (every size >= 1, fewer than 2^32 points): {L.lib.nero_last_error().decode()}')
    L.check_workspace_fits(need, dev, what='marching-cubes workspace')
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        s = L.stream_ptr()
        L.check(L.lib.nero_mcubes_count(L.ptr(u), nx, ny, nz, float(threshold), L.ptr(ws), L.ptr(totals), s))
        V, T = (int(x) for x in totals.tolist())
        if V >= _INT31 or T >= _INT31:
            raise L.NeroHipError(f'marching_cubes_device: {V} vertices / {T} triangles: the int32 triangle ids cannot hold them')
        L.check_workspace_fits(12 * (V + T), dev, what='marching-cubes mesh')
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((T, 3), dtype=torch.int32, device=dev)
        L.check(L.lib.nero_mcubes_emit(L.ptr(u), nx, ny, nz, float(threshold), L.ptr(ws), L.ptr(verts) if V else None, V,
                                       L.ptr(tris) if T else None, T, s))
    return verts, tris


def marching_cubes(volume, isovalue):
    """PyMCubes' `mcubes.marching_cubes(volume, isovalue)`: numpy [nx, ny, nz] -> (vertices float64 [V,3] in index space, triangles int64
    [T,3]), computed on the current CUDA device.  The volume is evaluated in float32 (the reference's grid is float32 already:
    extract_fields, network/field.py:1096)."""
    vol = torch.from_numpy(np.ascontiguousarray(np.asarray(volume), dtype=np.float32))
    v, f = marching_cubes_device(vol.cuda(), float(isovalue))
    return v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)


def index_to_world(verts, resolution, bound_min, bound_max):
    """the reference's mapping of index-space vertices to the box (network/field.py:1114-1116), in float64 on the host"""
    bmin = np.asarray(bound_min.detach().cpu().numpy() if torch.is_tensor(bound_min) else bound_min)
    bmax = np.asarray(bound_max.detach().cpu().numpy() if torch.is_tensor(bound_max) else bound_max)
    v = np.asarray(verts, dtype=np.float64)
    return v / (resolution - 1.0) * (bmax - bmin)[None, :] + bmin[None, :]


def index_to_world_device(verts, resolution, bound_min, bound_max):
    """index_to_world for a mesh that stays on the device: the same float64 expression, operation by operation, on the tensor's device,
    rounded to float32 -- the bits index_to_world(...).astype(float32) gives, which is what write_ply stores.  verts: CUDA tensor [V,3]"""
    bmin = np.asarray(bound_min.detach().cpu().numpy() if torch.is_tensor(bound_min) else bound_min)
    bmax = np.asarray(bound_max.detach().cpu().numpy() if torch.is_tensor(bound_max) else bound_max)
    span = torch.from_numpy(np.asarray(bmax - bmin, dtype=np.float64)).to(verts.device)
    base = torch.from_numpy(np.asarray(bmin, dtype=np.float64)).to(verts.device)
    return (verts.double() / (resolution - 1.0) * span[None, :] + base[None, :]).float().contiguous()


# ---- connected components and clean-up ---------------------------------------------------------------------------------------------------
class MeshComponents:
    """the connected components of a mesh (connected_components_device): K, and on the mesh's device label int32 [V] (the smallest vertex
    of each vertex's component), comp int32 [V] (the component of each vertex, numbered in ascending order of the smallest vertex), n_verts /
    n_faces int32 [K] (a face belongs to the component of its first vertex), area float64 [K], bbox_min / bbox_max float32 [K,3]"""
    __slots__ = ('K', 'label', 'comp', 'n_verts', 'n_faces', 'area', 'bbox_min', 'bbox_max')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def table(self):
        """-> one dict per component, on the host (for reports)"""
        cols = [getattr(self, k).tolist() for k in self.__slots__[3:]]
        return [{'component': i, 'n_verts': nv, 'n_faces': nf, 'area': a, 'bbox_min': lo, 'bbox_max': hi}
                for i, (nv, nf, a, lo, hi) in enumerate(zip(*cols))]


class CleanInfo:
    """what clean_mesh_device did: components (MeshComponents of the input), keep bool [K] (the components that stayed), vmap int32 [V]
    (the new index of every input vertex, -1 where it was dropped)"""
    __slots__ = ('components', 'keep', 'vmap')

    def __init__(self, components, keep, vmap):
        self.components, self.keep, self.vmap = components, keep, vmap


def _check_mesh(fn, verts, tris):
    ok_v = torch.is_tensor(verts) and verts.is_cuda and verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3
    ok_t = torch.is_tensor(tris) and tris.is_cuda and tris.dtype == torch.int32 and tris.dim() == 2 and tris.shape[1] == 3
    if not (ok_v and ok_t and verts.device == tris.device):
        d = lambda x: f'{tuple(x.shape)} {x.dtype} {x.device.type}' if torch.is_tensor(x) else type(x).__name__
        raise TypeError(f'{fn} wants CUDA float32 [V,3] vertices and CUDA int32 [T,3] triangles on one device, got {d(verts)} and {d(tris)}')
    if verts.shape[0] >= _INT31 or tris.shape[0] >= _INT31:
        raise L.NeroHipError(f'{fn}: {verts.shape[0]} vertices / {tris.shape[0]} triangles: 2^31 or more')
    return verts.contiguous(), tris.contiguous()


def connected_components_device(verts, tris):
    """verts CUDA float32 [V,3], tris CUDA int32 [T,3] -> MeshComponents.  Two vertices are connected when a triangle holds both; an
    unreferenced vertex is a component of its own with no face.  One readback of 16 bytes (K and the out-of-range flag) sizes the
    statistics.  A triangle index outside [0, V) raises ValueError (the kernels skip such a triangle, they never follow it)."""
    verts, tris = _check_mesh('connected_components_device', verts, tris)
    V, T = verts.shape[0], tris.shape[0]
    dev = verts.device
    need = int(L.lib.nero_mesh_cc_stats_workspace_bytes(V, T))
    if need == 0:
        raise L.NeroHipError(f'connected_components_device: {V} vertices / {T} triangles: no workspace ({L.lib.nero_last_error().decode()})')
    L.check_workspace_fits(need + 8 * V, dev, what='connected-components workspace')
    with torch.cuda.device(dev):
        s = L.stream_ptr()
        label = torch.empty(V, dtype=torch.int32, device=dev)
        info = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(L.lib.nero_mesh_cc_label(L.ptr(tris) if T else None, T, V, L.ptr(label) if V else None, L.ptr(info), s))
        K, bad = (int(x) for x in info.tolist())
        if bad:
            raise ValueError(f'connected_components_device: {bad} of {T} triangles hold a vertex index outside [0, {V})')
        comp = torch.empty(V, dtype=torch.int32, device=dev)
        out = MeshComponents(K=K, label=label, comp=comp, n_verts=torch.empty(K, dtype=torch.int32, device=dev),
                             n_faces=torch.empty(K, dtype=torch.int32, device=dev), area=torch.empty(K, dtype=torch.float64, device=dev),
                             bbox_min=torch.empty((K, 3), dtype=torch.float32, device=dev),
                             bbox_max=torch.empty((K, 3), dtype=torch.float32, device=dev))
        if V:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            L.check(L.lib.nero_mesh_cc_stats(L.ptr(verts), L.ptr(tris) if T else None, T, V, L.ptr(label), K, L.ptr(ws), L.ptr(comp),
                                             L.ptr(out.n_verts), L.ptr(out.n_faces), L.ptr(out.area), L.ptr(out.bbox_min),
                                             L.ptr(out.bbox_max), s))
    return out


def select_components(n_faces, keep=None, min_faces=0, min_face_ratio=0.0):
    """the selection rule of clean_mesh_device on the face counts n_faces [K] (a tensor on any device) -> bool [K].  keep: 'largest' (= 1) or
    an integer k: the k components with the most faces, ties towards the smaller component number; min_faces: at least that many faces;
    min_face_ratio: at least that fraction of the largest component's face count (compared in float64).  The rules intersect."""
    if keep == 'largest':
        keep = 1
    if keep is not None and (isinstance(keep, bool) or not isinstance(keep, int) or keep < 0):
        raise ValueError(f"keep must be None, 'largest' or a non-negative integer, got {keep!r}")
    if min_faces < 0 or not 0.0 <= min_face_ratio <= 1.0:
        raise ValueError(f'min_faces must be >= 0 and min_face_ratio in [0, 1], got {min_faces} and {min_face_ratio}')
    flags = torch.ones(n_faces.shape[0], dtype=torch.bool, device=n_faces.device)
    if n_faces.shape[0] == 0:
        return flags
    if keep is not None:
        order = torch.sort(n_faces, descending=True, stable=True).indices
        flags = torch.zeros_like(flags)
        flags[order[:keep]] = True
    if min_faces:
        flags &= n_faces >= int(min_faces)
    if min_face_ratio:
        flags &= n_faces.double() >= float(min_face_ratio) * n_faces.max().double()
    return flags


def clean_mesh_device(verts, tris, keep=None, min_faces=0, min_face_ratio=0.0):
    """verts CUDA float32 [V,3], tris CUDA int32 [T,3] -> (verts', tris', CleanInfo): the mesh without the components the rules reject
    (select_components) and without unreferenced vertices, the survivors in their original relative order.  With no rule only the
    unreferenced vertices go."""
    cc = connected_components_device(verts, tris)
    verts, tris = verts.contiguous(), tris.contiguous()
    V, T, K = verts.shape[0], tris.shape[0], cc.K
    dev = verts.device
    flags = select_components(cc.n_faces, keep, min_faces, min_face_ratio)
    need = int(L.lib.nero_mesh_compact_workspace_bytes(V, T))
    if need == 0:
        raise L.NeroHipError(f'clean_mesh_device: {V} vertices / {T} triangles: no workspace ({L.lib.nero_last_error().decode()})')
    L.check_workspace_fits(need, dev, what='mesh-compaction workspace')
    with torch.cuda.device(dev):
        s = L.stream_ptr()
        keep_u8 = flags.to(torch.uint8)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(L.lib.nero_mesh_compact_count(L.ptr(tris) if T else None, T, V, L.ptr(cc.comp) if V else None, L.ptr(keep_u8) if K else None,
                                              K, L.ptr(ws), L.ptr(totals), s))
        V2, T2 = (int(x) for x in totals.tolist())
        L.check_workspace_fits(12 * (V2 + T2) + 4 * V, dev, what='cleaned mesh')
        v2 = torch.empty((V2, 3), dtype=torch.float32, device=dev)
        f2 = torch.empty((T2, 3), dtype=torch.int32, device=dev)
        vmap = torch.empty(V, dtype=torch.int32, device=dev)
        L.check(L.lib.nero_mesh_compact_emit(L.ptr(verts) if V else None, L.ptr(tris) if T else None, T, V, L.ptr(ws), L.ptr(v2) if V2 else None,
                                             V2, L.ptr(f2) if T2 else None, T2, L.ptr(vmap) if V else None, s))
    return v2, f2, CleanInfo(cc, flags, vmap)


def clean_mesh(v, f, **rules):
    """clean_mesh_device on numpy arrays (e.g. what read_ply returns), computed on the current CUDA device: -> (vertices float64 [V',3],
    triangles int64 [T',3], CleanInfo).  The device works on a float32 copy of the vertices (statistics only: the clean-up selects, it
    computes no coordinate); the vertices returned are the caller's own rows, so float64 input keeps its bits."""
    v = np.asarray(v).reshape(-1, 3)
    f = np.asarray(f).reshape(-1, 3)
    if f.size and (f.min() < -_INT31 or f.max() >= _INT31):
        raise ValueError('clean_mesh: a face index does not fit int32')
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
    fd = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).cuda()
    _, f2, info = clean_mesh_device(vd, fd, **rules)
    kept = np.nonzero(info.vmap.cpu().numpy() >= 0)[0]
    return v[kept].astype(np.float64), f2.cpu().numpy().astype(np.int64), info


# ---- adjacency and charts ---------------------------------------------------------------------------------------------------------------
class ChartInfo:
    """the charts of a mesh (face_charts_device): K, and on the mesh's device chart_class int32 [K] (2 k + s: projected along axis k, onto the
    axes (k + 1) % 3 and (k + 2) % 3, mirrored when s = 1), n_faces int32 [K], box float32 [K,4] (min_p, min_q, max_p, max_q of the projected
    coordinates); n_boundary / n_nonmanifold (edges held by one face / by three or more), n_chartless (faces without a chart)"""
    __slots__ = ('K', 'chart_class', 'n_faces', 'box', 'n_boundary', 'n_nonmanifold', 'n_chartless')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _face_adjacency(tris, V):
    T = tris.shape[0]
    dev = tris.device
    need = int(L.lib.nero_mesh_face_adjacency_workspace_bytes(T))
    if T and need == 0:
        raise L.NeroHipError(f'face_adjacency_device: {T} triangles: no workspace ({L.lib.nero_last_error().decode()})')
    L.check_workspace_fits(need + 12 * T, dev, what='face-adjacency workspace')
    with torch.cuda.device(dev):
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        nbr = torch.empty((T, 3), dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(L.lib.nero_mesh_face_adjacency(L.ptr(tris) if T else None, T, int(V), L.ptr(ws), L.ptr(nbr) if T else None, L.ptr(counts),
                                               L.stream_ptr()))
    return nbr, counts


def face_adjacency_device(tris, n_verts):
    """tris CUDA int32 [T,3] over n_verts vertices -> (nbr int32 [T,3], n_boundary, n_nonmanifold): nbr[t, e] = the face on the other side of
    the edge (v_e, v_(e+1)%3) of face t when exactly two faces hold that edge, else -1; the edges held by one face and by three or more.  A
    face with an index outside [0, n_verts) or with a repeated index has no edges.  One readback of 16 bytes (the two counts)."""
    if not (torch.is_tensor(tris) and tris.is_cuda and tris.dtype == torch.int32 and tris.dim() == 2 and tris.shape[1] == 3):
        raise TypeError('face_adjacency_device wants CUDA int32 [T,3] triangles')
    if not 0 <= int(n_verts) < _INT31:
        raise L.NeroHipError(f'face_adjacency_device: {n_verts} vertices: negative, or 2^31 or more')
    nbr, counts = _face_adjacency(tris.contiguous(), n_verts)
    nb, nm = (int(x) for x in counts.tolist())
    return nbr, nb, nm


def face_charts_device(verts, tris):
    """verts CUDA float32 [V,3], tris CUDA int32 [T,3] -> (chart int32 [T], face_class int32 [T], nbr int32 [T,3], ChartInfo): the charts of
    the projection atlas.  A face's class is 2 k + (n_k < 0) for the largest component k of its float64 normal (6: no chart -- an index out
    of range or repeated, a normal that is zero or not finite); a chart is a set of faces of one class joined edge by edge (nbr as
    face_adjacency_device gives it); charts are numbered in ascending order of their smallest face, chartless faces get -1.  One readback
    of 32 bytes (K and the counts) sizes the per-chart arrays."""
    verts, tris = _check_mesh('face_charts_device', verts, tris)
    V, T = verts.shape[0], tris.shape[0]
    dev = verts.device
    nbr, counts = _face_adjacency(tris, V)
    need = int(L.lib.nero_mesh_chart_label_workspace_bytes(T))
    if need == 0:
        raise L.NeroHipError(f'face_charts_device: {T} triangles: no workspace ({L.lib.nero_last_error().decode()})')
    L.check_workspace_fits(need + 8 * T, dev, what='chart-label workspace')
    with torch.cuda.device(dev):
        s = L.stream_ptr()
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        cls = torch.empty(T, dtype=torch.int32, device=dev)
        chart = torch.empty(T, dtype=torch.int32, device=dev)
        info = torch.empty(2, dtype=torch.int64, device=dev)
        p = lambda x: L.ptr(x) if x.numel() else None
        L.check(L.lib.nero_mesh_chart_label(p(verts), p(tris), T, V, p(nbr), L.ptr(ws), p(cls), p(chart), L.ptr(info), s))
        K, chartless, nb, nm = (int(x) for x in torch.cat([info, counts]).tolist())
        out = ChartInfo(K=K, chart_class=torch.empty(K, dtype=torch.int32, device=dev), n_faces=torch.empty(K, dtype=torch.int32, device=dev),
                        box=torch.empty((K, 4), dtype=torch.float32, device=dev), n_boundary=nb, n_nonmanifold=nm, n_chartless=chartless)
        if K:
            L.check(L.lib.nero_mesh_chart_stats(L.ptr(verts), L.ptr(tris), T, V, L.ptr(chart), L.ptr(cls), K, L.ptr(out.chart_class),
                                                L.ptr(out.n_faces), L.ptr(out.box), s))
    return chart, cls, nbr, out


# ---- simplification ---------------------------------------------------------------------------------------------------------------------
SIMPLIFY_FACTORS = (1.0, 0.8408964152537145, 0.7071067811865476, 0.5946035575013605)      # 2^(-j/4)
SIMPLIFY_K_MAX = 80
_PLACEMENTS = {'mean': 0, 'quadric': 1}


def simplify_cells(D, k):
    """the cell sizes the face-budget search of simplify_mesh_device chooses from: D 2^-(k // 4) c[k % 4] in float64, k in [0, 80] (D: the
    longest side of the bounding box); four steps halve the cell"""
    k = int(k)
    if not 0 <= k <= SIMPLIFY_K_MAX:
        raise ValueError(f'simplify_cells: k must be in [0, {SIMPLIFY_K_MAX}], got {k}')
    return float(D) * 2.0 ** -(k // 4) * SIMPLIFY_FACTORS[k % 4]


class SimplifyInfo:
    """what simplify_mesh_device did: cell and origin (float, three floats) of the grid, k (the step of simplify_cells a face budget chose,
    else None), and on the mesh's device cell_key int64 [V'] (i_x << 42 | i_y << 21 | i_z of every output vertex, ascending), positions64
    float64 [V',3] (the positions as computed; the mesh carries their float32 rounding), vmap int32 [V] (the output vertex of each input
    vertex's cell, -1 when the cell is unused), fmap int32 [T] (the output index of each triangle that was kept, else -1), n_survivors (the
    triangles whose corners lie in three different cells), n_duplicates (the survivors the de-duplication removed)"""
    __slots__ = ('cell', 'origin', 'k', 'cell_key', 'positions64', 'vmap', 'fmap', 'n_survivors', 'n_duplicates')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


class _Simplifier:
    """one mesh, one workspace: the count calls of the face-budget search and the emit call share them"""

    def __init__(self, verts, tris, origin):
        self.verts, self.tris = verts, tris
        self.V, self.T = verts.shape[0], tris.shape[0]
        self.dev = verts.device
        self.origin = (C.c_double * 3)(*origin)
        need = int(L.lib.nero_mesh_simplify_workspace_bytes(self.V, self.T))
        if need == 0:
            raise L.NeroHipError(f'simplify_mesh_device: {self.V} vertices / {self.T} triangles: 2^31 or more vertices or corners')
        L.check_workspace_fits(need, self.dev, what='mesh-simplification workspace')
        self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        self.totals = torch.empty(4, dtype=torch.int32, device=self.dev)

    def count(self, cell, faces_only):
        """-> (V' or -1, survivors); one readback of 16 bytes.  Refused input raises ValueError"""
        V, T = self.V, self.T
        L.check(L.lib.nero_mesh_simplify_count(L.ptr(self.verts) if V else None, L.ptr(self.tris) if T else None, T, V, cell, self.origin,
                                               int(faces_only), L.ptr(self.ws), L.ptr(self.totals), L.stream_ptr()))
        v2, n, bad_v, bad_t = (int(x) for x in self.totals.tolist())
        if bad_v or bad_t:
            raise ValueError(f'simplify_mesh_device: {bad_v} of {V} vertices are non-finite or lie outside the 2^21 cells of size {cell} an '
                             f'axis holds from the origin {list(self.origin)}; {bad_t} of {T} triangles hold a vertex index outside [0, {V})')
        return v2, n


def simplify_mesh_device(verts, tris, cell=None, target_faces=None, origin=None, placement='quadric', dedup=True):
    """verts CUDA float32 [V,3], tris CUDA int32 [T,3] -> (verts', tris', SimplifyInfo): vertex clustering on the uniform grid of cells of
    size `cell` (in the units of verts; for the marching-cubes output: grid indices) from `origin` (default: the per-axis minimum of verts).
    A triangle survives when its corners lie in three different cells; the cells that hold a corner of a survivor become the vertices, in
    ascending cell order; the survivors keep their winding and relative order.  placement: 'quadric' puts a vertex where the planes of the
    triangles that touch the cell meet best (regularised towards the mean of the cell's vertices, clamped to the cell), 'mean' at that
    mean.  dedup: of several survivors with the same three vertices, in either winding, only the first stays.  target_faces=N instead of
    cell: the smallest cell of simplify_cells(D, k) that leaves at most N survivors, found by bisection over k with at most 8 counting
    passes (the survivor count is taken as non-decreasing in k); N below the count of k = 0 raises ValueError.
    Non-finite vertices, vertices more than 2^21 cells from the origin and triangle indices outside [0, V) raise ValueError naming their
    number (the kernels count them and never follow them).  Everything is bit-identical run to run."""
    verts, tris = _check_mesh('simplify_mesh_device', verts, tris)
    if (cell is None) == (target_faces is None):
        raise ValueError('simplify_mesh_device: give exactly one of cell and target_faces')
    if placement not in _PLACEMENTS:
        raise ValueError(f"simplify_mesh_device: placement must be 'quadric' or 'mean', got {placement!r}")
    if cell is not None and not (np.isfinite(float(cell)) and float(cell) > 0):
        raise ValueError(f'simplify_mesh_device: cell must be positive and finite, got {cell}')
    if target_faces is not None and (isinstance(target_faces, bool) or int(target_faces) != target_faces or target_faces < 0):
        raise ValueError(f'simplify_mesh_device: target_faces must be a non-negative integer, got {target_faces!r}')
    V, T = verts.shape[0], tris.shape[0]
    dev = verts.device
    with torch.cuda.device(dev):
        empty = lambda *shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        if V == 0 or T == 0:
            o = [0.0] * 3 if origin is None else [float(x) for x in origin]
            info = SimplifyInfo(cell=None if cell is None else float(cell), origin=o, k=None, cell_key=empty(0, dtype=torch.int64),
                                positions64=empty(0, 3, dtype=torch.float64), vmap=torch.full((V,), -1, dtype=torch.int32, device=dev),
                                fmap=torch.full((T,), -1, dtype=torch.int32, device=dev), n_survivors=0, n_duplicates=0)
            return empty(0, 3, dtype=torch.float32), empty(0, 3, dtype=torch.int32), info
        box = torch.stack([verts.amin(dim=0), verts.amax(dim=0)]).double().cpu()              # (float32 extrema are exact)
        finite = bool(torch.isfinite(box).all())
        if origin is None:
            origin = box[0].tolist() if finite else [0.0] * 3                                 # (the count below names the bad vertices)
        origin = [float(x) for x in origin]
        if len(origin) != 3 or not all(np.isfinite(origin)):
            raise ValueError(f'simplify_mesh_device: origin must be three finite numbers, got {origin}')
        job = _Simplifier(verts, tris, origin)
        k = None
        if target_faces is not None:
            if not finite:
                job.count(1.0, True)                                                          # raises, naming the count
            D = float((box[1] - box[0]).max())
            if not D > 0:
                raise ValueError('simplify_mesh_device: target_faces needs a mesh with a bounding box of positive size')
            n_of = lambda q: job.count(simplify_cells(D, q), True)[1]
            n0 = n_of(0)
            if n0 > target_faces:
                raise ValueError(f'simplify_mesh_device: target_faces = {target_faces} is below the {n0} faces the coarsest cell '
                                 f'({simplify_cells(D, 0)}) leaves')
            lo, hi = 0, SIMPLIFY_K_MAX + 1
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if n_of(mid) <= target_faces:
                    lo = mid
                else:
                    hi = mid
            k = lo
            cell = simplify_cells(D, k)
        cell = float(cell)
        V2, S = job.count(cell, False)
        L.check_workspace_fits(44 * V2 + 12 * S + 4 * (V + T), dev, what='simplified mesh')
        pos = empty(V2, 3, dtype=torch.float64)
        v2 = empty(V2, 3, dtype=torch.float32)
        key = empty(V2, dtype=torch.int64)
        f2 = empty(S, 3, dtype=torch.int32)
        vmap = empty(V, dtype=torch.int32)
        fmap = empty(T, dtype=torch.int32)
        n_out = empty(1, dtype=torch.int64)
        L.check(L.lib.nero_mesh_simplify_emit(L.ptr(verts), L.ptr(tris), T, V, cell, job.origin, _PLACEMENTS[placement], int(bool(dedup)),
                                              L.ptr(job.ws), L.ptr(pos) if V2 else None, L.ptr(v2) if V2 else None, L.ptr(key) if V2 else None,
                                              V2, L.ptr(f2) if S else None, S, L.ptr(vmap), L.ptr(fmap), L.ptr(n_out), L.stream_ptr()))
        T2 = int(n_out.item())
        if T2 < S:
            f2 = f2[:T2].clone()                                                              # (releases the survivors' capacity)
    return v2, f2, SimplifyInfo(cell=cell, origin=origin, k=k, cell_key=key, positions64=pos, vmap=vmap, fmap=fmap, n_survivors=S,
                                n_duplicates=S - T2)


def simplify_mesh(v, f, **kw):
    """simplify_mesh_device on numpy arrays (e.g. what read_ply returns), computed on the current CUDA device on a float32 copy of the
    vertices: -> (vertices float64 [V',3]: the float64 positions as computed, triangles int64 [T',3], SimplifyInfo)"""
    v = np.asarray(v).reshape(-1, 3)
    f = np.asarray(f).reshape(-1, 3)
    if f.size and (f.min() < -_INT31 or f.max() >= _INT31):
        raise ValueError('simplify_mesh: a face index does not fit int32')
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
    fd = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).cuda()
    _, f2, info = simplify_mesh_device(vd, fd, **kw)
    return info.positions64.cpu().numpy(), f2.cpu().numpy().astype(np.int64), info


# ---- vertex normals ---------------------------------------------------------------------------------------------------------------------
NORMAL_WEIGHTS = {'area': 0, 'angle': 1}


def _as_mesh(verts, tris, device=None):
    """host arrays or tensors on any device -> (verts float32 [V,3], tris int32 [T,3]) contiguous on `device` (None: where they are, host
    arrays on the host)"""
    v = verts.detach() if torch.is_tensor(verts) else torch.from_numpy(np.ascontiguousarray(np.asarray(verts), dtype=np.float32))
    t = tris.detach() if torch.is_tensor(tris) else torch.from_numpy(np.ascontiguousarray(np.asarray(tris), dtype=np.int32))
    if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'expected vertices [V, 3] and triangles [T, 3], got {tuple(v.shape)} and {tuple(t.shape)}')
    dev = v.device if device is None else device
    return v.to(device=dev, dtype=torch.float32).contiguous(), t.to(device=dev, dtype=torch.int32).contiguous()


def winding_sign(verts, tris):
    """+1 when the triangles of a closed mesh are wound so that their normals point outwards, -1 when inwards (the meshes of
    extract_mesh.py), 0 when the mesh encloses no volume (an open sheet): the sign of the signed volume sum p0 . (p1 x p2) over the faces,
    in float64 in torch after moving the centroid of the vertices to the origin, on the device the vertices are on.  Only the sign is used;
    a sum within the rounding noise of its terms (2^-40 of the sum of |p0| |p1| |p2|) counts as zero.  Faces with an index out of range or a
    non-finite corner are left out."""
    v, t = _as_mesh(verts, tris)
    t = t.to(v.device).long()
    V = v.shape[0]
    t = t[((t >= 0) & (t < V)).all(1)]
    p = v.double()
    finite = torch.isfinite(p).all(1)
    if not bool(finite.any()) or t.shape[0] == 0:
        return 0
    p = p - p[finite].mean(0, keepdim=True)
    c = p[t]                                                                               # [T,3,3]
    term = (c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum(1)
    size = c.norm(dim=2).prod(1)                                                           # |p0| |p1| |p2|: what a term's rounding scales with
    ok = torch.isfinite(term) & torch.isfinite(size)
    vol, noise = float(term[ok].sum()), float(size[ok].sum()) * 2.0 ** -40
    return 0 if abs(vol) <= noise else (1 if vol > 0 else -1)


def vertex_normals(verts, tris, weight='angle', orient='winding', return_info=False):
    """smooth per-vertex normals (nero_vertex_normals): verts [V,3], tris [T,3], host arrays or tensors -> float32 [V,3] on
    the device (that of the input tensors, else the current one).  weight: 'angle' (each face's unit normal weighted by its angle at the
    vertex: independent of how a surface is cut into triangles) or 'area' (by its area).  orient: 'winding' leaves the normals on the
    side the triangles' winding gives, 'outward' multiplies them by winding_sign (zeros for a mesh that encloses no volume).  The same
    bits on every run and for every order of the triangles.  A vertex no face reaches, or whose faces cancel, gets (0, 0, 0); a face
    with an index outside [0, V) or a non-finite corner contributes nothing.  return_info: also info int64 [4] on the device = (refused
    faces, faces without area, vertices written as zero, the exponent of the area scale)."""
    if weight not in NORMAL_WEIGHTS:
        raise ValueError(f"vertex_normals: weight must be 'angle' or 'area', got {weight!r}")
    if orient not in ('winding', 'outward'):
        raise ValueError(f"vertex_normals: orient must be 'winding' or 'outward', got {orient!r}")
    dev = next((x.device for x in (verts, tris) if torch.is_tensor(x) and x.is_cuda), None)
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else dev
    v, t = _as_mesh(verts, tris, dev)
    V, T = v.shape[0], t.shape[0]
    need = int(L.lib.nero_vertex_normals_workspace_bytes(V, T))
    if need == 0:
        raise L.NeroHipError(f'vertex_normals: {V} vertices / {T} triangles: {L.lib.nero_last_error().decode()}')
    L.check_workspace_fits(need + 12 * V, dev, what='vertex-normal workspace')
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        L.check(L.lib.nero_vertex_normals(L.ptr(v), V, L.ptr(t), T, NORMAL_WEIGHTS[weight], L.ptr(ws), L.ptr(out), L.ptr(info), L.stream_ptr()))
        if orient == 'outward':
            sign = winding_sign(v, t)
            if sign <= 0:
                out = out * float(sign) + 0.0                                              # (+ 0.0: a zero component stays +0, as the other winding's)
    return (out, info) if return_info else out


# ---- PLY --------------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def write_ply(path, v, f, normals=None):
    """binary little-endian PLY: `float x, y, z` per vertex, `list uchar int vertex_indices` per face (what trimesh writes for a mesh
    without attributes, extract_mesh.py:37).  normals [V,3]: `float nx, ny, nz` after z (vertex_normals); None: the same bytes as ever"""
    v = np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype='<f4').reshape(-1, 3)
    f = np.asarray(f.detach().cpu().numpy() if torch.is_tensor(f) else f).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError('write_ply: a face index is out of range')
    props = 'property float x\nproperty float y\nproperty float z\n'
    if normals is not None:
        n = np.ascontiguousarray(normals.detach().cpu().numpy() if torch.is_tensor(normals) else normals, dtype='<f4').reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError(f'write_ply: {len(n)} normals for {len(v)} vertices')
        v = np.ascontiguousarray(np.concatenate([v, n], 1))
        props += 'property float nx\nproperty float ny\nproperty float nz\n'
    faces = np.empty(len(f), dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    faces['n'] = 3
    faces['idx'] = f
    head = (f'ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\n{props}'
            f'element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n')
    with open(path, 'wb') as fh:
        fh.write(head.encode('ascii'))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())


def _read_header(fh):
    if fh.readline().strip() != b'ply':
        raise ValueError('read_ply: not a PLY file')
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError('read_ply: the header has no end_header')
        tok = line.decode('ascii', 'replace').split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'end_header':
            return fmt, elements
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append({'name': tok[1], 'count': int(tok[2]), 'props': []})
        elif tok[0] == 'property':
            if not elements:
                raise ValueError('read_ply: a property before any element')
            if tok[1] == 'list':
                elements[-1]['props'].append((tok[4], 'list', _ply_type(tok[2]), _ply_type(tok[3])))
            else:
                elements[-1]['props'].append((tok[2], _ply_type(tok[1])))


def _ply_type(name):
    if name not in _PLY_TYPES:
        raise ValueError(f'read_ply: unknown property type {name!r}')
    return _PLY_TYPES[name]


def _triangles(counts, where):
    bad = np.nonzero(np.asarray(counts) != 3)[0]
    if bad.size:
        raise ValueError(f'read_ply: face {int(bad[0])} of {where} has {int(np.asarray(counts)[bad[0]])} vertices; only triangle meshes are '
                         f'supported')


def read_ply(path, with_normals=False):
    """-> (vertices float64 [V,3], faces int64 [T,3]).  binary_little_endian or ascii; float or double x, y, z, other vertex properties
    (colours, ...) skipped; faces must be triangles.  Big-endian files and polygon faces raise ValueError.  with_normals: -> (vertices,
    faces, normals float32 [V,3] from the vertex properties nx, ny, nz, or None when the file has none)."""
    with open(path, 'rb') as fh:
        fmt, elements = _read_header(fh)
        if fmt == 'binary_big_endian':
            raise ValueError(f'read_ply: {os.path.basename(path)} is big-endian; only binary_little_endian and ascii PLY are supported')
        if fmt not in ('binary_little_endian', 'ascii'):
            raise ValueError(f'read_ply: unknown format {fmt!r}')
        body = fh.read()
    verts = faces = normals = None
    if fmt == 'ascii':
        lines = body.decode('ascii').split('\n')
        at = 0
        for el in elements:
            rows = [ln.split() for ln in lines[at:at + el['count']]]
            at += el['count']
            if el['name'] == 'vertex':
                cols = [p[0] for p in el['props']]
                if any(p[1] == 'list' for p in el['props']):
                    raise ValueError('read_ply: list properties on vertices are not supported')
                a = np.array(rows, dtype=np.float64).reshape(el['count'], len(cols))
                verts = a[:, [cols.index(c) for c in 'xyz']]
                if all(c in cols for c in ('nx', 'ny', 'nz')):
                    normals = a[:, [cols.index(c) for c in ('nx', 'ny', 'nz')]].astype(np.float32)
            elif el['name'] == 'face':
                if el['props'][0][1] != 'list':
                    raise ValueError('read_ply: the face element has no leading vertex-index list')
                _triangles([int(r[0]) for r in rows], path)
                faces = np.array([r[1:4] for r in rows], dtype=np.int64).reshape(el['count'], 3)
    else:
        at = 0
        for el in elements:
            if el['name'] == 'face':
                p0 = el['props'][0]
                if p0[1] != 'list' or any(p[1] == 'list' for p in el['props'][1:]):
                    raise ValueError('read_ply: faces must be one leading vertex-index list plus scalar properties')
                # one record per triangle: count, three indices, the remaining scalar properties
                dt = np.dtype([('n', '<' + p0[2]), ('idx', '<' + p0[3], (3,))] + [(p[0], '<' + p[1]) for p in el['props'][1:]])
                rec = np.frombuffer(body, dtype=dt, count=el['count'], offset=at) if el['count'] else np.zeros(0, dt)
                _triangles(rec['n'], path)                # (the first polygon's count is read at its true position: all before it were triangles)
                faces = rec['idx'].astype(np.int64)
                at += dt.itemsize * el['count']
            else:
                if any(p[1] == 'list' for p in el['props']):
                    raise ValueError(f'read_ply: list properties on element {el["name"]!r} are not supported in binary files')
                dt = np.dtype([(p[0], '<' + p[1]) for p in el['props']])
                rec = np.frombuffer(body, dtype=dt, count=el['count'], offset=at) if el['count'] else np.zeros(0, dt)
                if el['name'] == 'vertex':
                    verts = np.stack([rec[c].astype(np.float64) for c in 'xyz'], -1).reshape(el['count'], 3)
                    if all(c in rec.dtype.names for c in ('nx', 'ny', 'nz')):
                        normals = np.stack([rec[c].astype(np.float32) for c in ('nx', 'ny', 'nz')], -1).reshape(el['count'], 3)
                at += dt.itemsize * el['count']
    if verts is None or faces is None:
        raise ValueError(f'read_ply: {os.path.basename(path)} has no vertex or no face element')
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError('read_ply: a face index is out of range')
    return (verts, faces, normals) if with_normals else (verts, faces)
