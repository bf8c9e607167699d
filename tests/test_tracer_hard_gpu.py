"""GPU tier of the mesh tracer on the hard cases of tests/tracer_ref.py: every traversal kernel against the float32 model of the walk
(oracle/tracer_oracle.py::trace_walk32, run on the tree the library exports) BIT FOR BIT -- depth, position, normal, face, the any-hit flag.
The kernels are built without fast-math (IEEE division and square root) and write every fused multiply-add out, the model restates them
operation by operation: equality follows from the code.  tests/test_tracer_model_cpu.py holds the model to exhaustive search, so the two tiers
together hold the kernels to it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.tracer_oracle import trace_brute32, trace_walk32
from tests import tracer_ref as TR
from tests.test_bvh_build_gpu import _create, _export

pytestmark = pytest.mark.gpu


def _lib():
    from nero_amd import _lib as L
    return L


class _Tree:
    """a handle of the library over a mesh of tests/tracer_ref.py, from the host or the device builder, and its exported records"""

    def __init__(self, name, build):
        L = _lib()
        v, f = TR.mesh(name)
        if build == 'host':
            self.h = C.c_void_p()
            L.check(L.lib.nero_bvh_create(v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p), len(f), C.byref(self.h)))
        else:
            rc, self.h = _create(v.copy(), f.copy())                  # (the cached arrays are read-only)
            L.check(rc)
        self.info, self.nodes, self.tris = _export(self.h)
        self.root = self.info[3]
        self.face_of = np.zeros(len(f), np.int32)
        L.check(L.lib.nero_bvh_export_faces(self.h, self.face_of.ctypes.data_as(C.c_void_p)))

    def close(self):
        _lib().lib.nero_bvh_destroy(self.h)


@functools.lru_cache(maxsize=None)
def _all_rays(name):
    """the ray sets of a mesh, one after the other: (o, d) float32 [10 n, 3] (a count that is no multiple of 64)"""
    sets = [TR.rays(name, s) for s in TR.RAY_SETS]
    o, d = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    return o[:-7], d[:-7]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape
    bad = (g != w).reshape(len(g), -1).any(1)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {len(g)} rays differ from the model, first ray {int(np.argmax(bad))}: ' \
                          f'{got[int(np.argmax(bad))].tolist()} vs {want[int(np.argmax(bad))].tolist()}'


@pytest.mark.parametrize('build', ['host', 'device'])
@pytest.mark.parametrize('name', TR.MESHES)
def test_kernels_equal_the_model_bit_for_bit(name, build):
    L = _lib()
    o_np, d_np = _all_rays(name)
    n = len(o_np)
    assert n % 64 != 0 and n % 256 != 0
    o, d = torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()
    t = _Tree(name, build)
    try:
        M = trace_walk32(t.nodes, t.tris, t.root, o_np, d_np)
        assert (M['slot'] >= 0).mean() > 0.2
        want_face = np.where(M['slot'] >= 0, t.face_of[np.maximum(M['slot'], 0)], -1).astype(np.int32)
        any_model = {tmax: trace_walk32(t.nodes, t.tris, t.root, o_np, d_np, tmax=tmax, any_hit=True)['slot'] >= 0 for tmax in (0.05, 0.5, 10.0)}
        assert any_model[10.0].any() and not any_model[10.0].all()
        for mode in (0, 1):
            L.check(L.lib.nero_bvh_set_traversal(t.h, mode))
            where = f'{name}, {build} builder, traversal {mode}'
            pos, nrm, depth = torch.empty_like(o), torch.empty_like(o), torch.empty(n, device='cuda')
            L.check(L.lib.nero_bvh_trace(t.h, o.data_ptr(), d.data_ptr(), n, pos.data_ptr(), nrm.data_ptr(), depth.data_ptr(), L.stream_ptr()))
            _same(depth, M['depth'], f'nero_bvh_trace depth ({where})')
            _same(pos, M['pos'], f'nero_bvh_trace position ({where})')
            _same(nrm, M['nrm'], f'nero_bvh_trace normal ({where})')
            pos2, nrm2, depth2 = torch.empty_like(o), torch.empty_like(o), torch.empty(n, device='cuda')
            skip = torch.zeros(n, dtype=torch.uint8, device='cuda')
            L.check(L.lib.nero_bvh_trace_masked(t.h, o.data_ptr(), d.data_ptr(), n, skip.data_ptr(), pos2.data_ptr(), nrm2.data_ptr(),
                                                depth2.data_ptr(), L.stream_ptr()))
            _same(depth2, M['depth'], f'nero_bvh_trace_masked depth ({where})')
            _same(pos2, M['pos'], f'nero_bvh_trace_masked position ({where})')
            _same(nrm2, M['nrm'], f'nero_bvh_trace_masked normal ({where})')
            depth3, face = torch.empty(n, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
            bary = torch.empty(n, 2, device='cuda')
            L.check(L.lib.nero_bvh_trace_faces(t.h, o.data_ptr(), d.data_ptr(), n, depth3.data_ptr(), face.data_ptr(), bary.data_ptr(), L.stream_ptr()))
            _same(depth3, M['depth'], f'nero_bvh_trace_faces depth ({where})')
            assert np.array_equal(face.cpu().numpy(), want_face), f'nero_bvh_trace_faces face ({where})'
            for tmax, want in any_model.items():
                occ = torch.empty(n, dtype=torch.uint8, device='cuda')
                L.check(L.lib.nero_bvh_occluded(t.h, o.data_ptr(), d.data_ptr(), n, None, tmax, None, occ.data_ptr(), L.stream_ptr()))
                got = occ.cpu().numpy() != 0
                assert np.array_equal(got, want), f'nero_bvh_occluded below {tmax} ({where}): {int((got != want).sum())} rays differ from the model'
    finally:
        t.close()


@pytest.mark.parametrize('name', ['hf_flat', 'mc_sphere', 'box'])
def test_host_builder_tree_meets_exhaustive_search(name):
    """the host builder orders the triangles of a leaf differently from tests/bvh_build_ref.py, whose tree the CPU tier walks: the contract of
    tests/test_tracer_model_cpu.py -- hit or miss as exhaustive search, the depth that of an accepted triangle within 1e-5 of the nearest -- on
    the kernels' own answers over the host builder's tree, on the vertex-aimed and the axis-parallel rays"""
    L = _lib()
    t = _Tree(name, 'host')
    try:
        for ray_set in ('vertex', 'axis_vertex', 'axis_face'):
            o_np, d_np = TR.rays(name, ray_set)
            n = len(o_np)
            o, d = torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()
            B = trace_brute32(t.tris, o_np, d_np)
            depth3, face = torch.empty(n, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
            bary = torch.empty(n, 2, device='cuda')
            L.check(L.lib.nero_bvh_trace_faces(t.h, o.data_ptr(), d.data_ptr(), n, depth3.data_ptr(), face.data_ptr(), bary.data_ptr(), L.stream_ptr()))
            depth = depth3.cpu().numpy()
            keep = ~(B['t_outside'].astype(np.float64) <= B['depth'].astype(np.float64) + 1e-5)
            hb, hw = B['slot'] >= 0, depth < np.float32(TR.MISS)
            assert np.array_equal(hb[keep], hw[keep]), (name, ray_set, int((hb != hw)[keep].sum()))
            both = hb & hw & keep
            assert both.sum() > 1000
            assert ((B['acc_t'].view(np.uint32) == depth.view(np.uint32)[:, None]) & (B['acc_slot'] >= 0)).any(1)[both].all(), (name, ray_set)
    finally:
        t.close()
