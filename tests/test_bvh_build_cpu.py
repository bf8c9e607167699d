"""CPU tier of the device BVH build: the numpy restatement of the tree (tests/bvh_build_ref.py) against itself, the library's new symbols and
its workspace arithmetic, and the host planning header (nero_amd/csrc/bvh_build_plan.h) compiled into a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import bvh_build_ref as R
from tests.helpers import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('nero_bvh_build_workspace_bytes', 'nero_bvh_build_lds_capacity', 'nero_bvh_create_device', 'nero_bvh_info', 'nero_bvh_export')


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib as L
    return L.bind(ctypes.CDLL(os.path.join(ROOT, 'nero_amd', 'libnero_hip.so')))


def test_shape_of_the_tree_for_every_size():
    for nT in range(1, 3001):
        levels = R.shape_levels(nT)
        leaves = sorted((int(lo), int(n)) for L in levels for lo, n in zip(L['lo'][~L['inner']], L['n'][~L['inner']]))
        at = 0
        for lo, n in leaves:                                   # the leaves partition [0, nT), 1 .. 4 triangles each
            assert lo == at and 1 <= n <= 4
            at += n
        assert at == nT
        inner = [(int(lo), l, int(node), int(n)) for l, L in enumerate(levels) for lo, n, node in
                 zip(L['lo'][L['inner']], L['n'][L['inner']], L['node'][L['inner']])]
        n_nodes, _, max_depth, root = R.info(nT)
        assert len(inner) == n_nodes == R.inner_count(nT)
        assert [node for _, _, node, _ in sorted(inner)] == list(range(n_nodes))          # DFS pre-order: by start, then by level
        if nT > 4:
            assert max_depth == math.ceil(math.log2(nT / 4)) == max(l for _, l, _, _ in inner) + 1 and root == 0
        else:
            assert max_depth == 0 and root == -(nT) - 1
        for L in levels:
            assert len(np.unique(L['n'])) <= 2 and int(L['n'].max() - L['n'].min()) <= 1  # at most two sizes per level, one apart


def test_children_follow_the_pre_order_rule():
    from nero_amd.synthetic import icosphere
    v, f = icosphere(2, 0.5, 0.15)
    for nT in (5, 9, 37, 320):
        ref = R.build(v, f[:nT])
        nodes, (n_nodes, n_tris, max_depth, root) = ref['node_array'], ref['info']
        assert (n_nodes, n_tris, root) == (R.inner_count(nT), nT, 0) and sorted(ref['order']) == list(range(nT))
        assert not nodes['pad'].any()

        def walk(me, lo, n, depth):
            h = n // 2
            nd = nodes[me]
            assert nd['left'] == (R.leaf_ref(lo, h) if h <= 4 else me + 1)
            assert nd['right'] == (R.leaf_ref(lo + h, n - h) if n - h <= 4 else me + 1 + R.inner_count(h))
            d = depth
            if h > 4:
                d = max(d, walk(me + 1, lo, h, depth + 1))
            if n - h > 4:
                d = max(d, walk(me + 1 + R.inner_count(h), lo + h, n - h, depth + 1))
            return d
        assert walk(0, 0, nT, 1) == max_depth


def test_ties():
    # 10 copies of one triangle whose x is -0 or +0 in turn: all extents are 0, axis 0, and the order stays the index order
    tri = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)
    v = np.tile(tri[None], (10, 1, 1))
    v[::2, :, 0] = -0.0
    ref = R.build(v.reshape(-1, 3), np.arange(30, dtype=np.int32).reshape(10, 3))
    assert np.array_equal(ref['order'], np.arange(10))
    assert np.signbit(ref['node_array']['lmin'][0][0]) and not np.signbit(ref['node_array']['lmax'][0][0])      # -0 is the smaller zero
    # equal extents on all three axes take axis 0; a strictly larger later axis wins
    c = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    assert R.pick_axis(c) == 0 and R.pick_axis(c * np.float32([1, 2, 2])) == 1 and R.pick_axis(c * np.float32([1, 2, 3])) == 2
    # equal keys keep the order they had before the sort: 6 triangles, x centroids 1 0 1 0 1 0
    v = np.zeros((6, 3, 3), np.float32)
    v[:, :, 0] = np.float32([1, 0, 1, 0, 1, 0])[:, None]
    ref = R.build(v.reshape(-1, 3), np.arange(18, dtype=np.int32).reshape(6, 3))
    assert list(ref['order']) == [1, 3, 5, 0, 2, 4]


def test_library_exports_the_device_build():
    lib = _lib()
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, 'include', 'nero_hip.h')).read()
    assert all(n + '(' in hdr for n in NEW_SYMBOLS)
    assert lib.nero_bvh_build_lds_capacity() >= 8


def test_workspace_bytes_needs_no_device():
    lib = _lib()
    sizes = [1, 2, 4, 5, 100, 1023, 1024, 1025, 4099, 81920, 327680, 1 << 20, (1 << 20) + 1, 1 << 24, (1 << 27) - 1]
    got = [int(lib.nero_bvh_build_workspace_bytes(1000, n)) for n in sizes]
    assert all(g > 0 for g in got) and got == sorted(got)
    assert all(g >= 60 * n for g, n in zip(got, sizes))            # centroids, boxes, two orders and two key arrays
    assert lib.nero_bvh_build_workspace_bytes(1000, 1 << 27) == 0 and lib.nero_bvh_build_workspace_bytes(1000, 0) == 0
    assert lib.nero_bvh_build_workspace_bytes(2, 10) == 0


def test_planning_header_under_sanitizers(tmp_path):
    """bvh_build_plan.h as a stand-alone program, built with -fsanitize=address,undefined and run as a child process: its level tables, node
    counts, per-level walks and hand-off levels equal the restatement's for every nT in 1 .. 5000"""
    cap = _lib().nero_bvh_build_lds_capacity()
    for c in (cap, 16):                                           # the library's S, and a small one (more hand-off levels in range)
        lines = run_host_program(tmp_path, 'bvh_plan_main.cpp', args=('1', '5000', str(c))).splitlines()
        assert len(lines) == 5000
        for nT, line in zip(range(1, 5001), lines):
            assert line == R.plan_line(nT, c), nT
