"""Drop-in for the reference's `raytracing.RayTracer` (raytracing/raytracer.py:8-54): same constructor and trace() contract,
backed by the HIP BVH in libnero_hip.so instead of the un-vendored `_raytracing` CUDA extension."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


class RayTracer:
    """build='host' (default): the tree is built by the library's host builder from numpy arrays (nero_bvh_create).  build='device': the mesh
    stays (or is put) on the GPU and the same tree is built there (nero_bvh_create_device); `_v` / `_f` remain available as host arrays,
    copied on first access."""

    def __init__(self, vertices, triangles, build='host'):
        assert build in ('host', 'device'), build
        assert triangles.shape[0] > 8, "BVH needs at least 8 triangles."          # same guard as the reference wrapper (:16)
        self.build = build
        self._h = None                       # the device BVH is built on first use (construction works without a GPU)
        self._dv = self._df = None           # build='device': the mesh as CUDA tensors, from first use (or from the caller) on
        if build == 'device':
            self._src = (vertices.detach() if torch.is_tensor(vertices) else vertices,
                         triangles.detach() if torch.is_tensor(triangles) else triangles)
            self._host = None
            return
        if torch.is_tensor(vertices):
            vertices = vertices.detach().cpu().numpy()
        if torch.is_tensor(triangles):
            triangles = triangles.detach().cpu().numpy()
        self._host = (np.ascontiguousarray(vertices, dtype=np.float32), np.ascontiguousarray(triangles, dtype=np.int32))

    def _host_arrays(self):
        if self._host is None:               # build='device': one copy, on first access
            v, f = self._src
            v = v.cpu().numpy() if torch.is_tensor(v) else v
            f = f.cpu().numpy() if torch.is_tensor(f) else f
            self._host = (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32))
        return self._host

    @property
    def _v(self):
        return self._host_arrays()[0]

    @property
    def _f(self):
        return self._host_arrays()[1]

    def _device_arrays(self):
        if self._dv is None:
            v, f = self._src
            v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
            f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32))
            self._dv = v.to(device='cuda', dtype=torch.float32).contiguous()
            self._df = f.to(device='cuda', dtype=torch.int32).contiguous()
        return self._dv, self._df

    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            if self.build == 'device':
                v, f = self._device_arrays()
                need = int(L.lib.nero_bvh_build_workspace_bytes(int(v.shape[0]), int(f.shape[0])))
                if need == 0:
                    raise NotImplementedError(f'RayTracer(build="device"): no device build for {v.shape[0]} vertices, {f.shape[0]} triangles')
                with torch.cuda.device(v.device):
                    ws = torch.empty(need, dtype=torch.uint8, device=v.device)
                    L.check(L.lib.nero_bvh_create_device(v.data_ptr(), int(v.shape[0]), f.data_ptr(), int(f.shape[0]),
                                                         ws.data_ptr(), need, L.stream_ptr(), C.byref(h)))
                    ws.record_stream(torch.cuda.current_stream())         # (the build's kernels may still be using it when it is released)
            else:
                L.check(L.lib.nero_bvh_create(self._v.ctypes.data_as(C.c_void_p), self._v.shape[0], self._f.ctypes.data_as(C.c_void_p),
                                              self._f.shape[0], C.byref(h)))
            self._h = h
        return self._h

    def info(self):
        """{'n_nodes', 'n_tris', 'max_depth', 'root'} of the tree (nero_bvh_info); builds it if need be"""
        out = [C.c_int() for _ in range(4)]
        L.check(L.lib.nero_bvh_info(self._handle(), *[C.byref(x) for x in out]))
        return dict(zip(('n_nodes', 'n_tris', 'max_depth', 'root'), (int(x.value) for x in out)))

    def __del__(self):
        try:
            if getattr(self, '_h', None):
                L.lib.nero_bvh_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def trace_grouped(self, rays_o, rays_d, group, heavy_from, inplace=False):
        """trace() with a launch-order hint (nero_bvh_trace_grouped): rays in groups of `group`, entries [heavy_from, group) of every
        group started first (Stage II: the specular directions of a surface point).  Same outputs as trace()."""
        return self.trace(rays_o, rays_d, inplace, _order=(int(group), int(heavy_from)))

    def trace_masked(self, rays_o, rays_d, skip, inplace=False, chunk_order=None):
        """trace() that does not traverse the rays flagged in `skip` (uint8 tensor [n] or a device pointer, or None; nero_bvh_trace_masked): they
        are reported as misses.  Every other ray: the outputs of trace() bit for bit.  chunk_order: a permutation of range(k) -- the rays come
        in groups of 64 k and the launch starts chunk chunk_order[0] of every group first, then chunk_order[1], ... (nero_bvh_trace_ordered:
        same outputs, another launch order)."""
        return self.trace(rays_o, rays_d, inplace, _skip=skip, _chunks=chunk_order)

    def trace(self, rays_o, rays_d, inplace=False, _order=None, _skip=None, _chunks=None):
        rays_o = rays_o.float().contiguous()
        rays_d = rays_d.float().contiguous()
        if not rays_o.is_cuda:
            rays_o = rays_o.cuda()
        if not rays_d.is_cuda:
            rays_d = rays_d.cuda()
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.view(-1, 3)
        rays_d = rays_d.view(-1, 3)
        n = rays_o.shape[0]
        positions = rays_o if inplace else torch.empty_like(rays_o)
        face_normals = rays_d if inplace else torch.empty_like(rays_d)
        depth = torch.empty(n, dtype=torch.float32, device=rays_o.device)
        if inplace:                      # the kernel reads o/d before it writes: each thread owns its ray
            pass
        if torch.is_tensor(_skip):       # both masked routes read n bytes at this pointer (an integer device pointer is taken as given)
            assert _skip.dtype == torch.uint8 and _skip.is_cuda and _skip.device == rays_o.device and _skip.numel() == n \
                and _skip.is_contiguous()
        if _chunks is not None:
            sp = None if _skip is None else (_skip.data_ptr() if torch.is_tensor(_skip) else int(_skip))
            arr = (C.c_int * len(_chunks))(*[int(c) for c in _chunks])
            L.check(L.lib.nero_bvh_trace_ordered(self._handle(), rays_o.data_ptr(), rays_d.data_ptr(), n, sp, arr,
                                                 len(_chunks), positions.data_ptr(), face_normals.data_ptr(), depth.data_ptr(), L.stream_ptr()))
        elif _skip is not None:
            sp = _skip.data_ptr() if torch.is_tensor(_skip) else int(_skip)
            L.check(L.lib.nero_bvh_trace_masked(self._handle(), rays_o.data_ptr(), rays_d.data_ptr(), n, sp,
                                                positions.data_ptr(), face_normals.data_ptr(), depth.data_ptr(), L.stream_ptr()))
        elif _order is not None:
            L.check(L.lib.nero_bvh_trace_grouped(self._handle(), rays_o.data_ptr(), rays_d.data_ptr(), n,
                                                 positions.data_ptr(), face_normals.data_ptr(), depth.data_ptr(), _order[0], _order[1], L.stream_ptr()))
        else:
            L.check(L.lib.nero_bvh_trace(self._handle(), rays_o.data_ptr(), rays_d.data_ptr(), n,
                                         positions.data_ptr(), face_normals.data_ptr(), depth.data_ptr(), L.stream_ptr()))
        return positions.view(*prefix, 3), face_normals.view(*prefix, 3), depth.view(*prefix)

    def occluded(self, rays_o, rays_d, tmax=None, skip=None):
        """shadow rays (nero_bvh_occluded): uint8 tensor of the rays' leading shape, 1 where some triangle lies at 0 < t < tmax along the ray
        -- what `trace(...)[2] < tmax` says, without the walk to the closest hit.  tmax: None (10, the miss distance), a float in (0, 10],
        or a float32 CUDA tensor of the rays' leading shape (per ray, clamped to [0, 10]).  skip: uint8 CUDA tensor of that shape or None; a
        flagged ray reports 0 without a node visit."""
        rays_o = rays_o.float().contiguous()
        rays_d = rays_d.float().contiguous()
        if not rays_o.is_cuda:
            rays_o = rays_o.cuda()
        if not rays_d.is_cuda:
            rays_d = rays_d.cuda()
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.view(-1, 3)
        rays_d = rays_d.view(-1, 3)
        n = rays_o.shape[0]
        assert rays_d.shape[0] == n and rays_d.device == rays_o.device
        tp, tmax_all = None, 10.0
        if torch.is_tensor(tmax):
            assert tmax.dtype == torch.float32 and tmax.is_cuda and tmax.device == rays_o.device and tmax.is_contiguous() \
                and tmax.shape == prefix and tmax.numel() == n
            tp = tmax.data_ptr()
        elif tmax is not None:
            tmax_all = float(tmax)
        sp = None
        if skip is not None:
            assert torch.is_tensor(skip) and skip.dtype == torch.uint8 and skip.is_cuda and skip.device == rays_o.device \
                and skip.is_contiguous() and skip.shape == prefix and skip.numel() == n
            sp = skip.data_ptr()
        out = torch.empty(n, dtype=torch.uint8, device=rays_o.device)
        if n == 0:
            return out.view(*prefix)
        with torch.cuda.device(rays_o.device):
            L.check(L.lib.nero_bvh_occluded(self._handle(), rays_o.data_ptr(), rays_d.data_ptr(), n, tp, tmax_all, sp, out.data_ptr(),
                                            L.stream_ptr()))
        return out.view(*prefix)

    def closest(self, points, max_dist=None, sort=False):
        """exact point-to-mesh distance (nero_bvh_closest): -> (dist float32, face int32, bary float32 [..., 2], point float32 [..., 3]) of the
        points' leading shape -- the distance to the nearest point of the surface, the lowest face index among the faces that attain it, that
        point's weights (b1, b2) on the face's second and third corner, and the point itself.  max_dist: None (no limit) or a positive float;
        a point with nothing within it, or with a non-finite coordinate, reports face -1, dist +inf and zeros.  sort: the queries are put in
        the order of a 30-bit Morton key of their position before the call (neighbouring lanes then walk neighbouring subtrees) and the
        outputs back in the caller's order after it; the outputs are the same bits either way."""
        points = points.float().contiguous()
        if not points.is_cuda:
            points = points.cuda()
        prefix = points.shape[:-1]
        pts = points.view(-1, 3)
        n = pts.shape[0]
        dev = pts.device
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev)
        bary = torch.empty((n, 2), dtype=torch.float32, device=dev)
        point = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if n > 0:
            order = None
            if sort:
                order = torch.sort(_morton30(pts), stable=True)[1]
                pts = pts[order].contiguous()
            with torch.cuda.device(dev):
                L.check(L.lib.nero_bvh_closest(self._handle(), pts.data_ptr(), n, float('inf') if max_dist is None else float(max_dist),
                                               dist.data_ptr(), face.data_ptr(), bary.data_ptr(), point.data_ptr(), L.stream_ptr()))
            if order is not None:
                back = torch.empty_like(order)
                back[order] = torch.arange(n, device=dev)
                dist, face, bary, point = dist[back], face[back], bary[back], point[back]
        return dist.view(*prefix), face.view(*prefix), bary.view(*prefix, 2), point.view(*prefix, 3)


def _morton30(pts):
    """30-bit Morton key (10 bits per axis, over the points' own bounding box) of float32 points [n,3] -> int64 [n]; a non-finite coordinate
    counts as 0.  Plumbing for RayTracer.closest(sort=True): only the ORDER of the queries depends on it."""
    p = torch.nan_to_num(pts, nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = p.min(0).values, p.max(0).values
    q = ((p - lo) / (hi - lo).clamp_min(1e-30) * 1023.0).clamp(0, 1023).long()

    def spread(x):                      # abcdefghij -> a00b00c00d00e00f00g00h00i00j
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    return spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
