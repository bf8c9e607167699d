"""CPU tier: the marching-cubes case table on its own terms, the numpy restatement (tests/mcubes_ref.py) on analytic fields, PLY IO, and the
Stage-II renderer reading a .ply without trimesh."""
import sys

import numpy as np
import pytest

from tests import mcubes_ref as R


def _below(case):
    return [(case >> c) & 1 for c in range(8)]


def _midpoints():
    return {e: (R.CORNERS[a] + R.CORNERS[b]) / 2.0 for e, (a, b) in enumerate(R.EDGES)}


def _rows():
    return [[int(x) for x in R.TRI_TABLE[c][:3 * R.TRI_COUNT[c]]] for c in range(256)]


def test_table_edges_are_exactly_the_crossing_edges():
    for c, row in enumerate(_rows()):
        b = _below(c)
        crossing = {e for e, (p, q) in enumerate(R.EDGES) if b[p] != b[q]}
        assert set(row) == crossing, c


def test_table_counts_match_the_kernels_count_table():
    for c in range(256):
        n = int(np.argmax(R.TRI_TABLE[c] < 0)) if (R.TRI_TABLE[c] < 0).any() else 16
        assert n % 3 == 0 and n // 3 == R.TRI_COUNT[c], c
        assert (R.TRI_TABLE[c][n:] == -1).all(), c
    assert R.TRI_COUNT[0] == 0 and R.TRI_COUNT[255] == 0 and R.TRI_COUNT.max() == 5


def test_case_one_normal_points_at_corner_zero():
    P = _midpoints()
    a, b, c = R.TRI_TABLE[1][:3]
    assert (a, b, c) == (0, 8, 3)
    n = np.cross(P[b] - P[a], P[c] - P[a])
    assert np.allclose(n / np.abs(n).max(), [-1, -1, -1])


def test_every_triangle_faces_the_below_region():
    """orientation of every triangle of every case (midpoint vertices): its normal points from the above corners to the below corners of
    the edges it cuts"""
    P = _midpoints()
    for c, row in enumerate(_rows()):
        b = _below(c)
        for t in range(0, len(row), 3):
            e = row[t:t + 3]
            n = np.cross(P[e[1]] - P[e[0]], P[e[2]] - P[e[0]])
            s = sum(n @ (R.CORNERS[p] - R.CORNERS[q]) if b[p] else n @ (R.CORNERS[q] - R.CORNERS[p]) for p, q in (R.EDGES[k] for k in e))
            assert s > 0, (c, e)


def test_unambiguous_faces_get_matching_boundary_segments():
    """crack-freedom of the table: inside a cell every triangle edge is shared by two triangles in opposite directions or lies on a cube
    face; on every face whose corner pattern is not ambiguous, every case cuts the same segments, and the cell on the other side of the
    face cuts them in the opposite direction"""
    P = _midpoints()
    segs = {}
    for c, row in enumerate(_rows()):
        b = _below(c)
        de = {(row[t + i], row[t + (i + 1) % 3]) for t in range(0, len(row), 3) for i in range(3)}
        assert len(de) == len(row), c                                  # no directed edge twice
        boundary = [(p, q) for p, q in de if (q, p) not in de]
        for p, q in boundary:
            assert any(P[p][ax] == P[q][ax] and P[p][ax] in (0, 1) for ax in range(3)), (c, p, q)
        for ax in range(3):
            for side in (0, 1):
                on = sorted((i for i in range(8) if R.CORNERS[i][ax] == side), key=lambda i: tuple(np.delete(R.CORNERS[i], ax)))
                pattern = tuple(b[i] for i in on)
                s = frozenset((tuple(np.delete(P[p], ax)), tuple(np.delete(P[q], ax))) for p, q in boundary
                              if P[p][ax] == side and P[q][ax] == side)
                segs.setdefault((ax, pattern, side), set()).add(s)
    for (ax, pattern, side), ss in segs.items():
        if pattern in ((1, 0, 0, 1), (0, 1, 1, 0)):
            continue
        assert len(ss) == 1, (ax, pattern, side)
        other = segs[(ax, pattern, 1 - side)]
        assert {(q, p) for p, q in next(iter(ss))} == set(next(iter(other))), (ax, pattern, side)


@pytest.mark.parametrize('name', sorted(R.FIXTURES))
def test_reference_mesh_on_analytic_fields(name):
    make, chi, volume = R.FIXTURES[name]
    u = make()
    assert R.ambiguous_faces(u) == 0                                   # Bourke's table is crack-free off ambiguous faces only
    v, f = R.marching_cubes(u, 0.0)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert len(v) == R.crossing_edges(u)
    ok, _ = R.closed_oriented_report(f)
    assert ok
    assert R.euler_characteristic(v, f) == chi
    vol = R.signed_volume(v, f)
    assert vol < 0                                                     # inward winding
    assert abs(-vol / volume - 1) < 0.01, (vol, volume)
    assert np.isin(np.arange(len(v)), f).all()                         # every vertex is used


def test_reference_vertices_lie_on_their_edges():
    u = np.random.default_rng(3).uniform(-1, 1, (9, 7, 6)).astype(np.float32)
    u[2, 3, 4] = 0.0                                                   # exactly the threshold: above (strict rule)
    v, f = R.marching_cubes(u, 0.0)
    frac = v - np.floor(v)
    assert ((frac > 0).sum(1) <= 1).all()                              # at most one non-integer coordinate
    assert f.min() >= 0 and f.max() < len(v)
    assert R.marching_cubes(u[:1], 0.0)[0].shape == (0, 3)


def test_ply_binary_round_trip_is_exact(tmp_path):
    from nero_amd.mesh import read_ply, write_ply
    rg = np.random.default_rng(0)
    v = rg.normal(size=(500, 3)).astype(np.float32)
    f = rg.integers(0, 500, (900, 3)).astype(np.int64)
    p = str(tmp_path / 'm.ply')
    write_ply(p, v, f)
    head = open(p, 'rb').read(300)
    assert b'format binary_little_endian 1.0' in head and b'property list uchar int vertex_indices' in head
    v2, f2 = read_ply(p)
    assert v2.dtype == np.float64 and f2.dtype == np.int64
    assert np.array_equal(v2, v.astype(np.float64)) and np.array_equal(f2, f)


def test_ply_ascii_with_extra_properties(tmp_path):
    from nero_amd.mesh import read_ply
    text = ('ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty double nx\nproperty float x\nproperty float y\n'
            'property float z\nproperty uchar red\nelement face 2\nproperty list uchar int vertex_indices\nproperty uchar flags\nend_header\n'
            '0.5 0 0 0 255\n0.5 1 0 0 0\n-1 0 1 0 7\n0 0.25 0.5 -1.5 9\n3 0 1 2 1\n3 0 2 3 0\n')
    p = tmp_path / 'a.ply'
    p.write_text(text)
    v, f = read_ply(str(p))
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.5, -1.5]])
    assert np.array_equal(f, [[0, 1, 2], [0, 2, 3]])


def test_ply_binary_with_double_vertices_and_extra_properties(tmp_path):
    from nero_amd.mesh import read_ply
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.125]])
    vrec = np.zeros(3, dtype=[('x', '<f8'), ('y', '<f8'), ('z', '<f8'), ('nx', '<f4'), ('red', 'u1')])
    vrec['x'], vrec['y'], vrec['z'] = v.T
    frec = np.zeros(1, dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    frec['n'], frec['idx'] = 3, [2, 1, 0]
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\n'
            'property float nx\nproperty uchar red\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n')
    p = tmp_path / 'd.ply'
    p.write_bytes(head.encode() + vrec.tobytes() + frec.tobytes())
    v2, f2 = read_ply(str(p))
    assert np.array_equal(v2, v) and np.array_equal(f2, [[2, 1, 0]])


def test_ply_rejects_polygons_and_big_endian(tmp_path):
    from nero_amd.mesh import read_ply
    quad = ('ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n'
            'property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n')
    (tmp_path / 'q.ply').write_text(quad)
    with pytest.raises(ValueError, match='triangle'):
        read_ply(str(tmp_path / 'q.ply'))
    (tmp_path / 'b.ply').write_bytes(b'ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n')
    with pytest.raises(ValueError, match='big-endian'):
        read_ply(str(tmp_path / 'b.ply'))


def test_material_renderer_reads_ply_without_trimesh(tmp_path, monkeypatch):
    from nero_amd.mesh import write_ply
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import golden_mesh, load_golden
    v, f = golden_mesh()
    p = str(tmp_path / 'shape.ply')
    write_ply(p, v, f)
    monkeypatch.setitem(sys.modules, 'trimesh', None)                  # `import trimesh` raises ImportError
    _, meta = load_golden('mat_bell')
    net = NeROMaterialRenderer({'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell', 'mesh': p})
    assert net.ray_tracer._h is None                                   # (the BVH is built on first use: no GPU needed here)
    assert np.array_equal(net.ray_tracer._v, np.asarray(v, np.float32))
    assert np.array_equal(net.ray_tracer._f, np.asarray(f, np.int32))
    with pytest.raises(ImportError):
        NeROMaterialRenderer({'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell', 'mesh': str(tmp_path / 'shape.obj')})
