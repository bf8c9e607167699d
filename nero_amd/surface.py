"""Area-weighted sampling of points on a mesh's surface on the GPU (include/nero_hip_surface.h, nero_amd/csrc/surface_sample.hip; DESIGN.md
9.13): the step the reference's eval.md gives to CloudCompare ("sample points on the surface", 500k by default) between the mesh clean-up
(nero_amd.mesh.mesh_clean) and the Chamfer distance of eval_real_shape.py (nero_amd.eval_shape.eval_meshes).

Deterministic: the same mesh, n, seed and mode give the same bits on every run and for every `chunk`.  The areas are summed as INTEGER
weights, sample i is a function of (i, n, seed) alone, and no floating-point atomic is used."""
import os

import numpy as np
import torch

from . import _lib as L

MAX_SAMPLES = 2 ** 31 - 1
_lib = L.lib


def _mesh(vertices, triangles):
    """-> (as_numpy, device, verts [V,3] float32, tris [T,3] int32), both contiguous on the device"""
    as_numpy = not (torch.is_tensor(vertices) or torch.is_tensor(triangles))
    dev = next((t.device for t in (vertices, triangles) if torch.is_tensor(t) and t.is_cuda), None)
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else dev
    v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(np.asarray(vertices), dtype=np.float32))
    t = triangles if torch.is_tensor(triangles) else torch.from_numpy(np.ascontiguousarray(np.asarray(triangles), dtype=np.int32))
    if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f'expected vertices [V, 3] and triangles [T, 3], got {tuple(v.shape)} and {tuple(t.shape)}')
    if v.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError('a mesh without vertices or without triangles has no surface to sample')
    return as_numpy, dev, v.detach().to(device=dev, dtype=torch.float32).contiguous(), t.detach().to(device=dev, dtype=torch.int32).contiguous()


def _cdf(v, t):
    """-> (cdf [T] int64, info [4] int64), both on the device; nothing is read back"""
    T, dev = t.shape[0], v.device
    need = int(_lib.nero_surface_cdf_workspace_bytes(T))
    if need == 0:
        raise NotImplementedError(f'surface_cdf: {T} triangles are not supported: {_lib.nero_last_error().decode()}')
    with torch.cuda.device(dev):
        L.check_workspace_fits(need + 8 * T, dev, what='surface-sampling workspace')
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        cdf = torch.empty(T, dtype=torch.int64, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        L.check(_lib.nero_surface_cdf(L.ptr(v), v.shape[0], L.ptr(t), T, L.ptr(ws), L.ptr(cdf), L.ptr(info), L.stream_ptr()))
    return cdf, info


def _record(cdf, info):
    total, zero_weight, e, B = (int(x) for x in info.cpu().tolist())
    return {'cdf': cdf, 'info': info, 'total': total, 'zero_weight': zero_weight, 'e': e, 'B': B, 'area': total * 2.0 ** (e - B) / 2}


def surface_cdf(vertices, triangles):
    """the running sum of the triangles' integer weights (nero_surface_cdf) -> dict: cdf [T] int64 and info [4] int64 on the device, and on
    the host total (= cdf[-1]), zero_weight (triangles that can never be chosen: no area, an index out of range, a non-finite vertex), e, B
    (w[t] = floor(2 area[t] 2^(B - e))) and area = total 2^(e - B) / 2, the mesh's area up to the flooring of the weights.  Pass the dict
    to sample_surface(cdf=...) to sample one mesh several times."""
    _, _, v, t = _mesh(vertices, triangles)
    return _record(*_cdf(v, t))


def sample_surface(vertices, triangles, n, seed=0, stratified=True, return_face=False, return_bary=False, return_normals=False, cdf=None,
                   chunk=None):
    """n points on the surface, each triangle chosen in proportion to its area and the point uniform inside it -> points [n,3] float32, or
    the tuple (points, face [n] int32 if return_face, bary [n,2] float32 = the weights of the face's second and third corner if return_bary,
    normals [n,3] float32 = the face's unit normal in its winding's direction if return_normals).  numpy in -> numpy out, a device tensor in
    -> device tensors out.  stratified: one jittered sample per n-th of the total area (every triangle gets its expected count to within
    2), else n independent draws.  cdf: what surface_cdf returned for the same mesh; chunk: samples per kernel call (any value gives the
    same bits).  A mesh with no area raises ValueError."""
    n = int(n)
    if not 0 <= n <= MAX_SAMPLES:
        raise ValueError(f'sample_surface: n = {n} is outside [0, 2^31 - 1]')
    as_numpy, dev, v, t = _mesh(vertices, triangles)
    rec = _record(*_cdf(v, t)) if cdf is None else cdf
    if rec['cdf'].shape[0] != t.shape[0]:
        raise ValueError(f"sample_surface: a cdf of {rec['cdf'].shape[0]} triangles for a mesh of {t.shape[0]}")
    if rec['total'] == 0:
        raise ValueError(f"sample_surface: the mesh has no area (all {t.shape[0]} triangles have weight 0)")
    chunk = max(n, 1) if chunk is None else max(1, int(chunk))
    with torch.cuda.device(dev):
        pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev) if return_face else None
        bary = torch.empty(n, 2, dtype=torch.float32, device=dev) if return_bary else None
        nrm = torch.empty(n, 3, dtype=torch.float32, device=dev) if return_normals else None
        part = lambda x, i, m: None if x is None else L.ptr(x[i:i + m])
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            L.check(_lib.nero_surface_sample(L.ptr(v), v.shape[0], L.ptr(t), t.shape[0], L.ptr(rec['cdf']), L.ptr(rec['info']), i, m, n,
                                             int(seed) & 0xffffffff, int(bool(stratified)), part(pts, i, m), part(face, i, m),
                                             part(bary, i, m), part(nrm, i, m), L.stream_ptr()))
    out = [x for x in (pts, face, bary, nrm) if x is not None]
    if as_numpy:
        out = [x.cpu().numpy() for x in out]
    return out[0] if len(out) == 1 else tuple(out)
