"""numpy restatement of the geometry evaluation's contract (include/nero_hip.h, "geometry evaluation"): what the HIP kernels of
nero_amd/csrc/geom_eval.hip are held to.  TEST INFRASTRUCTURE ONLY.

back_project / nearest_dist / chamfer restate the reference's arithmetic (utils/base_utils.py:44-52, 562-565, 583-584,
eval_synthetic_shape.py:16-25, 91-95) and are pinned to its recorded outputs by tests/test_geom_eval_cpu.py (tests/golden/geom_eval.npz);
voxel_down_sample restates the deterministic form of open3d's voxel_down_sample that the header fixes."""
import numpy as np

AXIS_BITS = 21


def back_project(mask, depth, K, pose, offset=0.0):
    """mask_depth_to_pts(mask, depth, K) -> pose_apply(pose_inverse(pose), .) -> float32 [n,3] in np.nonzero (row-major) order.
    The pixel coordinates and the depth meet in a float32 array and x z, y z are float32 products; everything after that is float64.
    offset = 0 is the reference; 0.5 un-projects through the pixel centres."""
    K = np.asarray(K, np.float64)
    pose = np.asarray(pose, np.float64)
    hs, ws = np.nonzero(mask)
    z = np.asarray(depth, np.float32)[hs, ws]
    pts = np.stack([ws.astype(np.float32) + np.float32(offset), hs.astype(np.float32) + np.float32(offset), z], 1)
    pts[:, :2] *= pts[:, 2:]
    iK = np.linalg.inv(K)
    v = pts.astype(np.float64)
    pc = np.stack([v[:, 0] * iK[r, 0] + v[:, 1] * iK[r, 1] + v[:, 2] * iK[r, 2] for r in range(3)], 1)
    R = pose[:, :3]
    c = -(R.T @ pose[:, 3])
    pw = np.stack([pc[:, 0] * R[0, k] + pc[:, 1] * R[1, k] + pc[:, 2] * R[2, k] + c[k] for k in range(3)], 1)
    return pw.astype(np.float32)


def nearest_dist(pts0, pts1, batch=256, return_index=False):
    """float32: for every point of pts0 the minimum over pts1 of norm(p0 - p1), the difference formed first"""
    a = np.asarray(pts0, np.float32)
    b = np.asarray(pts1, np.float32)
    out = np.empty(len(a), np.float32)
    idx = np.empty(len(a), np.int64)
    for i in range(0, len(a), batch):
        d = a[i:i + batch, None, :] - b[None, :, :]
        d2 = (d * d).sum(-1, dtype=np.float32)
        j = d2.argmin(1)
        idx[i:i + batch] = j
        out[i:i + batch] = np.sqrt(d2[np.arange(len(j)), j])
    return (out, idx) if return_index else out


def nearest_dist64(pts0, pts1, batch=256):
    """float64 brute force on the float32 inputs -> (distances, indices)"""
    a = np.asarray(pts0, np.float32).astype(np.float64)
    b = np.asarray(pts1, np.float32).astype(np.float64)
    out = np.empty(len(a))
    idx = np.empty(len(a), np.int64)
    for i in range(0, len(a), batch):
        d = a[i:i + batch, None, :] - b[None, :, :]
        d2 = (d * d).sum(-1)
        j = d2.argmin(1)
        idx[i:i + batch] = j
        out[i:i + batch] = np.sqrt(d2[np.arange(len(j)), j])
    return out, idx


def chamfer(pts_pr, pts_gt, nn=nearest_dist):
    dist_gt = nn(pts_gt, pts_pr)
    dist_pr = nn(pts_pr, pts_gt)
    return (np.mean(dist_gt) + np.mean(dist_pr)) / 2


def voxel_indices(points, voxel):
    """-> int64 [n,3]: floor((p - o) / voxel) in float64, o = min(points) - voxel / 2 per axis"""
    p = np.asarray(points, np.float32)
    o = p.min(0).astype(np.float64) - float(voxel) / 2
    return np.floor((p.astype(np.float64) - o) / float(voxel)).astype(np.int64), o


def voxel_down_sample(points, voxel, return_parts=False):
    """-> float32 [m,3]: per occupied voxel, in ascending order of the key ix << 42 | iy << 21 | iz, the float64 sum of its points taken in
    ascending input index (np.bincount accumulates in input order), divided by the count.  return_parts: also (keys [m], counts [m], voxel id
    of every input point [n], float64 means [m,3])."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if len(p) == 0:
        e = np.zeros((0, 3), np.float32)
        return (e, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3))) if return_parts else e
    ijk, _ = voxel_indices(p, voxel)
    if ijk.max() >= 1 << AXIS_BITS:
        raise NotImplementedError('more than 2^21 voxels on an axis')
    key = ijk[:, 0] << (2 * AXIS_BITS) | ijk[:, 1] << AXIS_BITS | ijk[:, 2]
    keys, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    mean = np.stack([np.bincount(inv, weights=p[:, a].astype(np.float64), minlength=len(keys)) for a in range(3)], 1) / counts[:, None]
    out = mean.astype(np.float32)
    return (out, keys, counts, inv, mean) if return_parts else out


def sphere_depth(K, pose, h, w, radius):
    """analytic depth map of the sphere |p| = radius seen through the pixel centres: (depth float32 [h,w] camera-space z, mask bool [h,w])"""
    K = np.asarray(K, np.float64)
    pose = np.asarray(pose, np.float64)
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
    dc = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    R, t = pose[:, :3], pose[:, 3]
    c = -(R.T @ t)
    dw = dc @ R
    a = (dw * dw).sum(-1)
    b = dw @ c
    disc = b * b - a * (c @ c - radius * radius)
    mask = disc > 0
    s = (-b - np.sqrt(np.where(mask, disc, 0.0))) / a                 # p = c + s dw, camera-space z = s dc_z = s
    return np.where(mask, s * dc[..., 2], 0.0).astype(np.float32), mask


def trace_chunk(args):
    """hit distances of oracle.tracer_oracle.trace_bruteforce for one chunk of rays (a picklable entry for worker processes)"""
    from oracle.tracer_oracle import trace_bruteforce
    v, f, o, d = args
    return trace_bruteforce(v, f, o, d)[2]
