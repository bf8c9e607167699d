"""Connected-component clean-up of the Stage-I mesh on one MI355X: label, statistics, compaction (HIP events, median over --reps after a
warm-up) and the whole clean_mesh_device call (wall clock: it holds the two 16-byte read-backs), on the marching-cubes mesh of the model
bench.py's inference_bench and scripts/bench_mesh.py use (seed 6033, perturb_state at variance 0.5).  Beside them the host route on the same
box in the same run: copy the mesh to the host, scipy.sparse.csgraph.connected_components, numpy statistics and compaction, copy the result
back.  A last row does the same on the marching-cubes mesh of a seeded white-noise grid (--noise).  Prints one JSON line and writes it to
profiles/bench_mesh_clean.json.

    python scripts/bench_mesh_clean.py [--res 256 512] [--reps 20] [--noise 160] [--no-write]

Bytes of the kernels, from the shapes (V vertices, T triangles, V' / T' surviving): label reads tris (12 T), writes and flattens parent
(12 V) and touches the parents of three vertices per triangle (12 T, the find / hook steps of a compressed forest); stats reads label and
writes comp, flags and ranks (20 V), reads the vertices for the boxes (12 V), reads tris twice and the vertices of every face for the
areas (24 T + 36 T), moves sort keys and values (16 T per radix pass; the pass count depends on K and is not modelled: one pass) and
reads the sorted face ids (4 T); compact reads tris twice (24 T), marks and scans the flags (16 V + 16 T), reads comp per face (4 T), copies the
surviving vertices (12 V + 12 V') and writes the map (4 V) and the remapped triangles (12 T' + 12 T' of vertex-rank reads)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
HBM_TBS = 6.3          # achievable HBM rate of one MI355X (measuring guide), TB/s


def byte_model(V, T, V2, T2):
    label = 12 * T + 12 * V + 12 * T
    stats = 20 * V + 12 * V + 24 * T + 36 * T + 16 * T + 4 * T
    compact = 24 * T + 16 * V + 16 * T + 4 * T + 12 * V + 12 * V2 + 4 * V + 24 * T2
    return {'label': label, 'stats': stats, 'compact': compact, 'total': label + stats + compact}


def kernels(verts, tris, reps):
    """label / stats / compact on the device mesh, HIP events; -> dict"""
    from nero_amd import _lib as L
    from nero_amd import mesh as M
    V, T = verts.shape[0], tris.shape[0]
    dev = verts.device
    label = torch.empty(V, dtype=torch.int32, device=dev)
    comp = torch.empty(V, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    ws_s = torch.empty(int(L.lib.nero_mesh_cc_stats_workspace_bytes(V, T)), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(int(L.lib.nero_mesh_compact_workspace_bytes(V, T)), dtype=torch.uint8, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    rows = []
    for it in range(reps + 3):
        s = L.stream_ptr()
        ev[0].record()
        L.check(L.lib.nero_mesh_cc_label(L.ptr(tris), T, V, L.ptr(label), L.ptr(info), s))
        ev[1].record()
        K, bad = info.tolist()
        assert bad == 0
        st = [torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev),
              torch.empty(K, dtype=torch.float64, device=dev), torch.empty((K, 3), dtype=torch.float32, device=dev),
              torch.empty((K, 3), dtype=torch.float32, device=dev)]
        ev[2].record()
        L.check(L.lib.nero_mesh_cc_stats(L.ptr(verts), L.ptr(tris), T, V, L.ptr(label), K, L.ptr(ws_s), L.ptr(comp), *[L.ptr(x) for x in st], s))
        ev[3].record()
        keep = M.select_components(st[1], keep='largest').to(torch.uint8)
        ev[4].record()
        L.check(L.lib.nero_mesh_compact_count(L.ptr(tris), T, V, L.ptr(comp), L.ptr(keep), K, L.ptr(ws_c), L.ptr(totals), s))
        V2, T2 = totals.tolist()
        v2 = torch.empty((V2, 3), dtype=torch.float32, device=dev)
        f2 = torch.empty((T2, 3), dtype=torch.int32, device=dev)
        L.check(L.lib.nero_mesh_compact_emit(L.ptr(verts), L.ptr(tris), T, V, L.ptr(ws_c), L.ptr(v2), V2, L.ptr(f2), T2, L.ptr(vmap), s))
        ev[5].record()
        torch.cuda.synchronize()
        if it >= 3:                                                    # (warm-up: code objects, allocator)
            rows.append((ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), ev[4].elapsed_time(ev[5])))
        del v2, f2, st
    med = [statistics.median(r[i] for r in rows) for i in range(3)]
    nb = byte_model(V, T, V2, T2)
    tot = sum(med)
    return {'V': V, 'T': T, 'K': K, 'V_kept': V2, 'T_kept': T2, 'reps': reps, 'label_ms': round(med[0], 4), 'stats_ms': round(med[1], 4),
            'compact_ms': round(med[2], 4), 'kernels_ms': round(tot, 4), 'bytes': nb,
            'GBps': round(nb['total'] / (tot * 1e-3) / 1e9, 1), 'frac_of_hbm': round(nb['total'] / (tot * 1e-3) / (HBM_TBS * 1e12), 4),
            'workspace_bytes': ws_s.numel() + ws_c.numel()}


def wall_median(fn, reps):
    out = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if it >= 1:
            out.append(time.perf_counter() - t0)
    return statistics.median(out), r


def host_route(verts, tris):
    """the mesh to the host, scipy's connected components, numpy selection of the largest component and compaction, the result back"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v, f = verts.cpu().numpy(), tris.cpu().numpy()
    V = len(v)
    a = np.concatenate([f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    K, lab = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(V, V)), directed=False)
    n_faces = np.bincount(lab[f[:, 0]], minlength=K)
    fk = lab[f[:, 0]] == int(np.argmax(n_faces))
    used = np.zeros(V, bool)
    used[f[fk].ravel()] = True
    vmap = np.cumsum(used, dtype=np.int32) - 1
    return torch.from_numpy(v[used]).to(verts.device), torch.from_numpy(vmap[f[fk]]).to(verts.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--noise', type=int, default=160, help='edge of the white-noise grid of the last row (0: skip it)')
    ap.add_argument('--no-write', action='store_true')
    args = ap.parse_args()
    from bench_mesh import model
    from nero_amd import mesh as M
    dev = torch.device('cuda:0')
    net = model(dev)
    net.extract_geometry(resolution=64, clean={'keep': 'largest'})    # warm-up (packing, allocator, code objects)
    out = {'metric': 'stage1_mesh_clean', 'device': torch.cuda.get_device_name(0), 'hbm_TBps_achievable': HBM_TBS}

    def measure(verts, tris, host_reps):
        r = kernels(verts, tris, args.reps)
        d_dev, (v2, f2, _) = wall_median(lambda: M.clean_mesh_device(verts, tris, keep='largest'), args.reps)
        d_host, (vh, fh) = wall_median(lambda: host_route(verts, tris), host_reps)
        assert torch.equal(f2, fh) and torch.equal(v2, vh)              # both routes give the same mesh
        r['clean_mesh_device_ms'] = round(d_dev * 1e3, 4)
        r['host_route_ms'] = round(d_host * 1e3, 4)
        r['device_faster_than_host'] = bool(d_dev < d_host)
        r['host_over_device'] = round(d_host / d_dev, 1)
        return r

    for res in args.res:
        with torch.no_grad():
            u = net._sdf_grid((-1., -1., -1.), (1., 1., 1.), res, 2 ** 21, 1.0)
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        out[f'{res}^3'] = measure(verts, tris, args.host_reps)
        del verts, tris
        torch.cuda.empty_cache()
    if args.noise:
        # the model's surface is smooth and small (one component).  White noise is the other end: millions of triangles in thousands of
        # components beside one that holds most of them -- the size and the contention the union-find has to stand
        g = torch.Generator(device=dev).manual_seed(6033)
        u = torch.rand((args.noise,) * 3, generator=g, device=dev) * 2 - 1
        verts, tris = M.marching_cubes_device(u, 0.0)
        del u
        out[f'noise_{args.noise}^3'] = measure(verts, tris, 1)
        del verts, tris
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(ROOT, 'profiles', 'bench_mesh_clean.json'), 'w') as fh_:
            fh_.write(line + '\n')


if __name__ == '__main__':
    main()
