"""Geometry evaluation of the extracted Stage-I mesh on the device: the reference's Chamfer procedure (eval_synthetic_shape.py,
eval_real_shape.py, eval.md) through libnero_hip.so (include/nero_hip.h, "geometry evaluation") instead of nvdiffrast, open3d and trimesh.

Function contracts follow the reference's:
  * nearest_dist(pts0, pts1, batch_size)            eval_synthetic_shape.py:16-25 (exact brute force, float32, no [batch, M, 3] tensor)
  * render_depth(mesh_or_tracer, pose, K, shape)    rasterize_depth_map, :39-60 -- by ray casting through pixel centres with the BVH tracer
  * mesh_eval_points / depth_eval_points            get_mesh_eval_points, :62-84 / get_database_eval_points, dataset/database.py:435-458
  * voxel_down_sample(points, voxel_size)           open3d's voxel_down_sample with a defined output order (ascending voxel key)
  * chamfer / eval_mesh / eval_point_clouds         main(), :86-97, and eval_real_shape.py:15-26
DEVIATION: nvdiffrast rasterises (screen-affine z, top-left fill rule); ray casting returns the true depth at the pixel centre and can differ
from it on boundary pixels.  nvdiffrast is not available to this project, so the difference is not measured.  Everything downstream of the
depth map follows the reference's own arithmetic, including its use of INTEGER pixel coordinates when un-projecting (unproject_offset = 0.0: a
half-pixel shift that its ground-truth points share; 0.5 puts every point on the ray it was traced along)."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from .raytracing import RayTracer

MISS_DISTANCE = 10.0                    # nero_bvh_trace reports a miss as depth 10

_lib = L.lib
_D9, _D12 = C.c_double * 9, C.c_double * 12


def _device(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _points(p, dev):
    """[n,3] float32 contiguous on dev, from numpy or a tensor (cast as the reference casts: astype(float32))"""
    if not torch.is_tensor(p):
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(p), dtype=np.float32))
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f'expected points [n, 3], got {tuple(p.shape)}')
    return p.to(device=dev, dtype=torch.float32).contiguous()


def _cam(K, pose):
    K = np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, dtype=np.float64)
    pose = np.asarray(pose.detach().cpu().numpy() if torch.is_tensor(pose) else pose, dtype=np.float64)
    if K.shape != (3, 3) or pose.shape != (3, 4):
        raise ValueError(f'expected K [3, 3] and pose [3, 4], got {K.shape} and {pose.shape}')
    return K, pose, _D9(*K.reshape(-1)), _D12(*pose.reshape(-1))


# ---- nearest neighbour / Chamfer -----------------------------------------------------------------------------------------------------------
def nn_splits(nq, nr):
    """over how many workgroups nearest_dist divides pts1 when `splits` is not given (nero_nn_dist_splits)"""
    return int(_lib.nero_nn_dist_splits(int(nq), int(nr)))


def nearest_dist(pts0, pts1, batch_size=None, return_index=False, splits=0):
    """for every point of pts0 the distance to its nearest point of pts1: float32 [n0].  numpy in -> numpy out (the reference's contract,
    eval_synthetic_shape.py:16-25; `batch_size` is accepted and ignored: nothing is batched); device tensors in -> device tensors out.
    return_index: also the index of that point (int32 on the device, int64 in numpy), the lowest among equally near ones.  splits: launch
    shape (0 = automatic); the result does not depend on it."""
    as_numpy = not (torch.is_tensor(pts0) or torch.is_tensor(pts1))
    dev = _device(pts0, pts1)
    q, r = _points(pts0, dev), _points(pts1, dev)
    nq, nr = q.shape[0], r.shape[0]
    if nr == 0 and nq > 0:
        raise ValueError('nearest_dist: pts1 is empty: the nearest distance is undefined')
    need = int(_lib.nero_nn_dist_workspace_bytes(nq, nr, int(splits)))
    if need == 0:
        raise ValueError(f'nearest_dist: splits = {splits} is not supported')
    with torch.cuda.device(dev):
        L.check_workspace_fits(need, dev, what='nearest-neighbour workspace')
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        dist = torch.empty(nq, dtype=torch.float32, device=dev)
        idx = torch.empty(nq, dtype=torch.int32, device=dev) if return_index else None
        L.check(_lib.nero_nn_dist(L.ptr(q), nq, L.ptr(r), nr, L.ptr(ws), int(splits), L.ptr(dist), L.ptr(idx), L.stream_ptr()))
    if as_numpy:
        dist = dist.cpu().numpy()
        idx = idx.cpu().numpy().astype(np.int64) if return_index else None
    return (dist, idx) if return_index else dist


def chamfer(pts_pr, pts_gt):
    """-> (chamfer, dist_gt, dist_pr): dist_gt = nearest_dist(gt, pr), dist_pr = nearest_dist(pr, gt) as float32 numpy arrays, and
    (np.mean(dist_gt) + np.mean(dist_pr)) / 2 with the means taken by numpy on the host (eval_synthetic_shape.py:91-95)"""
    dev = _device(pts_pr, pts_gt)
    pr, gt = _points(pts_pr, dev), _points(pts_gt, dev)
    dist_gt = nearest_dist(gt, pr).cpu().numpy()
    dist_pr = nearest_dist(pr, gt).cpu().numpy()
    return (np.mean(dist_gt) + np.mean(dist_pr)) / 2, dist_gt, dist_pr


def eval_point_clouds(pts_pr, pts_gt):
    """the Chamfer distance of two point sets (eval_real_shape.py:15-26 applies it to the vertices of two PLY files)"""
    return float(chamfer(pts_pr, pts_gt)[0])


def point_to_mesh(points, mesh_or_tracer, bvh_build='host', sort=True):
    """for every point its distance to the nearest point of the mesh's SURFACE (RayTracer.closest, nero_bvh_closest): float32 [n], exact up
    to float32 rounding -- no floor from a sample spacing, unlike nearest_dist against samples of the mesh.  numpy in -> numpy out, a tensor in
    -> a device tensor out (nearest_dist's contract).  mesh_or_tracer: as render_depth takes it; pass a RayTracer to reuse one tree.  sort:
    the launch order of the queries (RayTracer.closest); the result does not depend on it."""
    as_numpy = not torch.is_tensor(points)
    rt, _ = _tracer(mesh_or_tracer, bvh_build)
    dist = rt.closest(_points(points, _device(points)), sort=sort)[0]
    return dist.cpu().numpy() if as_numpy else dist


def eval_meshes(pr_mesh, gt_mesh, n=500000, seed=0, stratified=True, exact=False, bvh_build='host'):
    """the real-shape procedure from two MESHES, each a (vertices, triangles) pair: eval.md samples 500k points on the surface of the
    predicted and of the ground-truth mesh alike (there with CloudCompare, here with nero_amd.surface.sample_surface: area-weighted,
    deterministic in n and seed) before eval_real_shape.py takes the Chamfer distance of the two point sets.  exact: the same two sample
    sets, each measured to the OTHER MESH'S SURFACE (point_to_mesh; CloudCompare's cloud-to-mesh distance) instead of to the other set's
    nearest sample, then (mean + mean) / 2 on the host as chamfer takes its means: no floor from the sample spacing."""
    from .surface import sample_surface
    dev = _device(*pr_mesh, *gt_mesh)
    cloud = lambda m: sample_surface(_points(m[0], dev), m[1], n, seed=seed, stratified=stratified)      # (device tensors: nothing comes back)
    if not exact:
        return eval_point_clouds(cloud(pr_mesh), cloud(gt_mesh))
    dist_gt = point_to_mesh(cloud(gt_mesh), tuple(pr_mesh), bvh_build).cpu().numpy()
    dist_pr = point_to_mesh(cloud(pr_mesh), tuple(gt_mesh), bvh_build).cpu().numpy()
    return float((np.mean(dist_gt) + np.mean(dist_pr)) / 2)


# ---- voxel down-sampling -------------------------------------------------------------------------------------------------------------------
def voxel_down_sample(points, voxel_size, capacity=None):
    """one point per occupied voxel: the mean of the voxel's points (float64 sum in input order), voxels in ascending (ix, iy, iz) order with
    origin min(points) - voxel_size / 2 -- open3d's voxel_down_sample with a defined order.  numpy in -> float32 numpy out, device tensor in ->
    device tensor out.  capacity: rows to allocate for the output (default: one per input point, which always fits)."""
    as_numpy = not torch.is_tensor(points)
    dev = _device(points)
    p = _points(points, dev)
    n = p.shape[0]
    cap = n if capacity is None else int(capacity)
    need = int(_lib.nero_voxel_downsample_workspace_bytes(n))
    if need == 0:
        raise NotImplementedError(f'voxel_down_sample: {n} points are not supported: {L.lib.nero_last_error().decode()}')
    with torch.cuda.device(dev):
        L.check_workspace_fits(need + 12 * cap, dev, what='voxel down-sampling workspace')
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev)
        n_out = torch.zeros(1, dtype=torch.int64, device=dev)
        L.check(_lib.nero_voxel_downsample(L.ptr(p), n, float(voxel_size), L.ptr(ws), L.ptr(out), cap, L.ptr(n_out), L.stream_ptr()))
        out = out[:int(n_out.item())].clone()
    return out.cpu().numpy() if as_numpy else out


# ---- depth maps and eval points --------------------------------------------------------------------------------------------------------------
def _tracer(mesh_or_tracer, bvh_build='host'):
    """-> (RayTracer, vertices float32 numpy).  Accepts a RayTracer, a (vertices, triangles) pair, or an object with .vertices / .faces.
    bvh_build: where a tracer made here builds its tree (RayTracer(build=...))"""
    m = mesh_or_tracer
    if isinstance(m, RayTracer):
        return m, m._v
    if isinstance(m, (tuple, list)) and len(m) == 2:
        v, f = m
    elif hasattr(m, 'vertices') and hasattr(m, 'faces'):
        v, f = np.asarray(m.vertices), np.asarray(m.faces)
    else:
        raise TypeError('expected a RayTracer, a (vertices, triangles) pair or a mesh with .vertices and .faces')
    rt = RayTracer(v, f, build=bvh_build)
    return rt, rt._v


def _check_reach(verts, pose, what):
    """the tracer reports a miss at distance 10: geometry that far from the camera would silently drop out of the depth map"""
    if len(verts) == 0:
        return
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    centre = -(pose[:, :3].T @ pose[:, 3])
    far = np.sqrt((np.maximum(np.abs(centre - lo), np.abs(centre - hi)) ** 2).sum())
    if not far < MISS_DISTANCE:
        raise ValueError(f"{what}: the camera centre is {far:.3f} from the farthest corner of the mesh's bounding box; the tracer reports hits "
                         f"at distance >= {MISS_DISTANCE:g} as misses.  Scale the scene (mesh and camera translations) down.")


def view_rays(pose, K, shape, device=None):
    """primary rays of one view through its pixel centres -> (rays_o [h*w,3], rays_d [h*w,3] unit) float32 on the device, row-major"""
    h, w = int(shape[0]), int(shape[1])
    _, _, Kc, Pc = _cam(K, pose)
    dev = device or _device()
    with torch.cuda.device(dev):
        o = torch.empty((h * w, 3), dtype=torch.float32, device=dev)
        d = torch.empty((h * w, 3), dtype=torch.float32, device=dev)
        L.check(_lib.nero_view_rays(Kc, Pc, h, w, L.ptr(o), L.ptr(d), L.stream_ptr()))
    return o, d


def _view(rt, verts, pose, K, shape, unproject_offset, want_points):
    h, w = int(shape[0]), int(shape[1])
    Kn, Pn, Kc, Pc = _cam(K, pose)
    _check_reach(verts, Pn, 'render_depth')
    dev = _device()
    o, d = view_rays(Pn, Kn, (h, w), dev)
    _, _, t = rt.trace(o, d)
    need = int(_lib.nero_view_points_workspace_bytes(h, w))
    if need == 0:
        raise ValueError(f'render_depth: a view of {h} x {w} pixels is not supported: {L.lib.nero_last_error().decode()}')
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        depth = torch.empty((h, w), dtype=torch.float32, device=dev)
        mask = torch.empty((h, w), dtype=torch.uint8, device=dev)
        cap = h * w if want_points else 0
        pts = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev)
        n_pts = torch.zeros(1, dtype=torch.int64, device=dev)
        L.check(_lib.nero_view_points(L.ptr(t), Kc, Pc, h, w, float(unproject_offset), L.ptr(ws), L.ptr(depth), L.ptr(mask), L.ptr(pts), cap,
                                      L.ptr(n_pts), L.stream_ptr()))
        if want_points:
            pts = pts[:int(n_pts.item())]
    return depth, mask, pts


def render_depth(mesh_or_tracer, pose, K, shape, as_numpy=True, bvh_build='host'):
    """rasterize_depth_map's contract (eval_synthetic_shape.py:39-60): -> (depth float32 [h,w] camera-space z, mask bool [h,w]), by casting one
    ray through every pixel centre with the BVH tracer.  Pass a RayTracer to reuse one BVH across views.  Raises ValueError when the mesh
    reaches the tracer's miss distance (10) from the camera."""
    rt, verts = _tracer(mesh_or_tracer, bvh_build)
    depth, mask, _ = _view(rt, verts, pose, K, shape, 0.0, False)
    mask = mask.bool()
    return (depth.cpu().numpy(), mask.cpu().numpy()) if as_numpy else (depth, mask)


def depth_points(depth, mask, pose, K, unproject_offset=0.0):
    """mask_depth_to_pts + pose_inverse + pose_apply for one depth map: world points float32 [n,3] on the device, row-major pixel order"""
    dev = _device(depth, mask)
    dpt = (depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(np.asarray(depth), dtype=np.float32)))
    dpt = dpt.to(device=dev, dtype=torch.float32).contiguous()
    msk = (mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0)))
    msk = (msk != 0).to(device=dev, dtype=torch.uint8).contiguous()
    if dpt.dim() != 2 or msk.shape != dpt.shape:
        raise ValueError(f'expected depth and mask [h, w], got {tuple(dpt.shape)} and {tuple(msk.shape)}')
    h, w = dpt.shape
    _, _, Kc, Pc = _cam(K, pose)
    need = int(_lib.nero_view_points_workspace_bytes(h, w))
    if need == 0:
        raise ValueError(f'depth_points: a view of {h} x {w} pixels is not supported: {L.lib.nero_last_error().decode()}')
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pts = torch.empty((h * w, 3), dtype=torch.float32, device=dev)
        n_pts = torch.zeros(1, dtype=torch.int64, device=dev)
        L.check(_lib.nero_depth_points(L.ptr(dpt), L.ptr(msk), Kc, Pc, h, w, float(unproject_offset), L.ptr(ws), L.ptr(pts), h * w, L.ptr(n_pts),
                                       L.stream_ptr()))
        return pts[:int(n_pts.item())]


def _down(parts, voxel_size, dev):
    cloud = torch.cat(parts, 0) if parts else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    return cloud if voxel_size is None else voxel_down_sample(cloud, voxel_size)


def mesh_eval_points(vertices, triangles, poses, Ks, shapes, voxel_size=0.01, unproject_offset=0.0, bvh_build='host'):
    """get_mesh_eval_points (eval_synthetic_shape.py:62-84): the mesh's depth map in every view, back-projected, concatenated on the device
    and voxel-down-sampled once -> float32 [m,3] device tensor.  shapes: one (h, w) for all views or one per view; voxel_size None: the
    raw concatenated cloud.  bvh_build='device': the tracer's tree is built on the GPU (the mesh may be CUDA tensors)."""
    rt = RayTracer(vertices, triangles, build=bvh_build)
    shapes = np.asarray(shapes).reshape(-1, 2)
    parts = []
    for i, (pose, K) in enumerate(zip(poses, Ks)):
        parts.append(_view(rt, rt._v, pose, K, shapes[i % len(shapes)], unproject_offset, True)[2])
    return _down(parts, voxel_size, _device())


def depth_eval_points(depths, masks, poses, Ks, voxel_size=0.01, unproject_offset=0.0):
    """get_database_eval_points (dataset/database.py:441-456) for given ground-truth depth maps and masks -> float32 [m,3] device tensor"""
    parts = [depth_points(d, m, pose, K, unproject_offset) for d, m, pose, K in zip(depths, masks, poses, Ks)]
    return _down(parts, voxel_size, _device())


def eval_mesh(vertices, triangles, poses, Ks, shapes, gt_points=None, gt_depths=None, gt_masks=None, voxel_size=0.01, unproject_offset=0.0,
              bvh_build='host'):
    """the synthetic procedure (eval_synthetic_shape.py main): Chamfer distance between the mesh's eval points and the ground truth, given
    either as points (the data set's eval_pts.ply) or as per-view depth maps + masks"""
    if (gt_points is None) == (gt_depths is None):
        raise ValueError('eval_mesh: give the ground truth either as gt_points or as gt_depths + gt_masks')
    pr = mesh_eval_points(vertices, triangles, poses, Ks, shapes, voxel_size, unproject_offset, bvh_build)
    if gt_points is None:
        if gt_masks is None:
            raise ValueError('eval_mesh: gt_depths needs gt_masks')
        gt_points = depth_eval_points(gt_depths, gt_masks, poses, Ks, voxel_size, unproject_offset)
    return eval_point_clouds(pr, gt_points)


# ---- PLY point clouds ------------------------------------------------------------------------------------------------------------------------
def read_ply_points(path):
    """the `x y z` of a PLY file's vertex element, float64 [n,3]: point clouds without faces (eval_pts.ply) and the vertices of meshes alike.
    ascii or binary_little_endian, float or double coordinates, other scalar vertex properties skipped."""
    from .mesh import _read_header
    with open(path, 'rb') as fh:
        fmt, elements = _read_header(fh)
        if fmt not in ('binary_little_endian', 'ascii'):
            raise ValueError(f'read_ply_points: {os.path.basename(path)}: format {fmt!r}; only binary_little_endian and ascii PLY are supported')
        body = fh.read()
    at = 0
    lines = body.decode('ascii', 'replace').split('\n') if fmt == 'ascii' else None
    for el in elements:
        if el['name'] != 'vertex':
            if any(p[1] == 'list' for p in el['props']):
                raise ValueError(f'read_ply_points: element {el["name"]!r} with list properties comes before the vertices')
            at += el['count'] if fmt == 'ascii' else el['count'] * np.dtype([(p[0], '<' + p[1]) for p in el['props']]).itemsize
            continue
        if any(p[1] == 'list' for p in el['props']):
            raise ValueError('read_ply_points: list properties on vertices are not supported')
        cols = [p[0] for p in el['props']]
        if not all(c in cols for c in 'xyz'):
            raise ValueError(f'read_ply_points: {os.path.basename(path)}: the vertex element has no x, y, z')
        if fmt == 'ascii':
            rows = [ln.split() for ln in lines[at:at + el['count']]]
            a = np.array(rows, dtype=np.float64).reshape(el['count'], len(cols))
            return a[:, [cols.index(c) for c in 'xyz']]
        dt = np.dtype([(p[0], '<' + p[1]) for p in el['props']])
        rec = np.frombuffer(body, dtype=dt, count=el['count'], offset=at) if el['count'] else np.zeros(0, dt)
        return np.stack([rec[c].astype(np.float64) for c in 'xyz'], -1).reshape(el['count'], 3)
    raise ValueError(f'read_ply_points: {os.path.basename(path)} has no vertex element')


def write_ply_points(path, points, double=False):
    """binary little-endian PLY with a vertex element only (`float` or `double` x, y, z): what open3d writes for eval_pts.ply"""
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    p = np.ascontiguousarray(p, dtype='<f8' if double else '<f4').reshape(-1, 3)
    t = 'double' if double else 'float'
    with open(path, 'wb') as fh:
        fh.write(f'ply\nformat binary_little_endian 1.0\nelement vertex {len(p)}\nproperty {t} x\nproperty {t} y\nproperty {t} z\nend_header\n'
                 .encode('ascii'))
        fh.write(p.tobytes())
