"""CPU tier of the vertex normals (include/nero_hip_normals.h, nero_amd/csrc/mesh_normals.hip, nero_amd.mesh.vertex_normals): the
restatement (tests/normals_ref.py) against analysis -- spheres, a cube, permutations, reversal, cancelling faces --, the entry points'
refusals before any device call, the limit arithmetic under the sanitizers, the PLY round trip with normals and winding_sign.  The
header's binding: tests/test_binding_cpu.py."""
import numpy as np
import pytest

from tests import normals_ref as NR
from tests.helpers import run_host_program

ERR_ARG = -1
T_MAX = 2 ** 31 - 2
MODES = ('area', 'angle')


@pytest.fixture(scope='module')
def M():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import mesh
    return mesh


def _icosphere(*a, **kw):
    from nero_amd.synthetic import icosphere
    return icosphere(*a, **kw)


def _radial(v):
    r = np.asarray(v, np.float64)
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the restatement against analysis ----------------------------------------------------------------------------------------------------
def test_smooth_normals_of_a_sphere_lie_close_to_the_radius():
    """icosphere(3, 0.5): the worst angle to the radial direction is below 0.35 degrees for angle weights and 0.75 for area weights
    (measured 0.299 and 0.677), both below a fifth of the flat normals' 5.45"""
    v, f = _icosphere(3, 0.5)
    r = _radial(v)
    fn = NR.face_normals(v, f)
    flat = max(NR.worst_angle_deg(fn, r[f[:, i]]) for i in range(3))
    worst = {w: NR.worst_angle_deg(NR.vertex_normals(v, f, w)[0], r) for w in MODES}
    print('flat', flat, worst)
    assert 5.4 < flat < 5.5
    assert worst['angle'] < 0.35 and worst['area'] < 0.75
    assert worst['angle'] < flat / 5 and worst['area'] < flat / 5
    v2, f2 = _icosphere(2, 0.5)
    assert NR.worst_angle_deg(NR.vertex_normals(v2, f2, 'angle')[0], _radial(v2)) < 0.65
    assert NR.worst_angle_deg(NR.vertex_normals(v2, f2, 'area')[0], _radial(v2)) < 1.4


@pytest.mark.parametrize('subdiv', [0, 1])
def test_symmetric_spheres_give_the_radial_direction(subdiv):
    """every vertex of the icosahedron and of its first subdivision sees a symmetric ring of faces: the sum is radial up to the rounding of
    the fixed-point terms (2^-40 relative), so a component is the float32 rounding of the radial one or its neighbour: within 2^-24 below 1"""
    v, f = _icosphere(subdiv, 0.5)
    r = _radial(v)
    for w in MODES:
        n, info = NR.vertex_normals(v, f, w)
        assert info[:3].tolist() == [0, 0, 0]
        assert np.abs(n.astype(np.float64) - r).max() <= 2.0 ** -24


def test_cube_corners_in_angle_mode():
    """the two triangles of a face split its right angle at two corners and leave it whole at the others: every face gives every one of
    its corners 90 degrees in all, and the three faces at a corner sum to (+-1, +-1, +-1) pi / 2"""
    v, f = NR.cube()
    assert np.all((NR.face_normals(v, f) * v[f].mean(1)).sum(1) > 0)                        # wound outwards
    n, info = NR.vertex_normals(v, f, 'angle')
    assert info.tolist() == [0, 0, 0, 0]
    assert np.abs(n.astype(np.float64) - v / np.sqrt(3.0)).max() <= 2.0 ** -24
    sums, _ = NR.vertex_sums(v, f, 'angle')
    B = NR.term_bits(len(f), NR.ANGLE)
    assert B == 40 and np.abs(sums - np.rint(v.astype(np.float64) * np.pi / 2 * 2.0 ** B)).max() <= 6      # six corner terms, each rounded once
    # area weights count triangles, not faces: a corner that holds one triangle of one face and two of another leans (why angle is the default)
    assert np.abs(NR.vertex_normals(v, f, 'area')[0].astype(np.float64) - v / np.sqrt(3.0)).max() > 0.1


@pytest.mark.parametrize('weight', MODES)
def test_the_order_of_the_triangles_changes_no_bit(weight):
    v, f = _icosphere(3, 0.5, bumps=0.05)
    n, info = NR.vertex_normals(v, f, weight)
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(len(f))
        n2, info2 = NR.vertex_normals(v, f[perm], weight)
        assert np.array_equal(_bits(n), _bits(n2)) and np.array_equal(info, info2)


@pytest.mark.parametrize('weight', MODES)
def test_reversing_the_winding_flips_the_sign_bits_and_nothing_else(weight):
    """c changes sign exactly, the angles do not change at all (a and b swap: |a x b| and a . b are symmetric), rint is odd: every sum is
    negated exactly.  A component whose sum is zero is +0 / l = +0 under both windings, the one pattern whose sign stays."""
    v, f = _icosphere(3, 0.5, bumps=0.05)
    n, info = NR.vertex_normals(v, f, weight)
    n2, info2 = NR.vertex_normals(v, f[:, ::-1], weight)
    assert np.array_equal(info, info2)
    s, _ = NR.vertex_sums(v, f, weight)
    s2, _ = NR.vertex_sums(v, f[:, ::-1], weight)
    assert np.array_equal(s, -s2)
    flip = np.where(s != 0, np.uint32(0x80000000), np.uint32(0))
    assert np.array_equal(_bits(n2), _bits(n) ^ flip)
    assert (s != 0).mean() > 0.99


@pytest.mark.parametrize('weight', MODES)
def test_coincident_faces_of_opposite_winding_cancel(weight):
    v = np.asarray([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.7, 0.9]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 2, 1]], np.int32)
    n, info = NR.vertex_normals(v, f, weight)
    assert not n.any() and not np.signbit(n).any()
    assert info[:3].tolist() == [0, 0, 3]
    one, info1 = NR.vertex_normals(v, f[:1], weight)
    assert info1[2] == 0 and np.array_equal(_bits(one[0]), _bits(one[1])) and np.array_equal(_bits(one[0]), _bits(one[2]))
    assert abs(float(np.linalg.norm(one[0].astype(np.float64))) - 1) < 1e-7


def test_refused_and_degenerate_faces_are_counted_and_silent():
    v, f = _icosphere(1, 0.5)
    v2, f2, keep = NR.spoiled(v, f)
    for weight in MODES:
        n, info = NR.vertex_normals(v, f, weight)
        n2, info2 = NR.vertex_normals(v2, f2, weight)
        assert np.array_equal(_bits(n2[keep]), _bits(n))
        assert not n2[len(v):].any()
        assert info2[:3].tolist() == [4, 1, 2] and info2[3] == info[3]


# ---- 2. the surface: refusals (the binding: tests/test_binding_cpu.py) ----------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device(M):
    from nero_amd import _lib as L
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    # nero_vertex_normals(verts, V, tris, T, weight, ws, normals, info, stream)
    call = lambda **kw: lib.nero_vertex_normals(*[kw.get(k, d) for k, d in (
        ('verts', p), ('V', 8), ('tris', p), ('T', 4), ('weight', 1), ('ws', p), ('normals', p), ('info', p), ('stream', None))])
    for V, T in ((8, 0), (2 ** 31 - 1, 4), (0, 4), (8, -1), (-1, 4), (8, T_MAX + 1), (2 ** 33 + 8, 4), (8, 2 ** 33 + 7)):
        assert call(V=V, T=T) == ERR_ARG and 'V and T must be in [1, 2^31 - 2]' in err(), (V, T)
    for weight in (2, -1, 3):
        assert call(weight=weight) == ERR_ARG and 'weight must be 0 (area) or 1 (angle)' in err()
    for k in ('normals', 'verts', 'tris', 'ws', 'info'):
        assert call(**{k: None}) == ERR_ARG and 'nero_vertex_normals: null pointer' in err()
    assert call(ws=p + 8) == ERR_ARG and 'aligned' in err()
    for V, T in ((8, 2 ** 33 + 7), (8, 0), (0, 8), (T_MAX + 1, 8), (8, T_MAX + 1)):
        assert lib.nero_vertex_normals_workspace_bytes(V, T) == 0 and '[1, 2^31 - 2]' in err()
    assert lib.nero_vertex_normals_workspace_bytes(1, 1) == 512
    assert lib.nero_vertex_normals_workspace_bytes(T_MAX, T_MAX) == 256 + 24 * T_MAX + 48          # 24 (2^31 - 2) is 208 past a multiple of 256
    with pytest.raises(ValueError, match='weight'):
        M.vertex_normals(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), weight='uniform')
    with pytest.raises(ValueError, match='orient'):
        M.vertex_normals(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), orient='inward')


# ---- 3. limits ------------------------------------------------------------------------------------------------------------------------------
def test_limit_arithmetic_under_the_sanitizers(tmp_path):
    """nero_amd/csrc/normals_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program): B at T = 1, 2^21,
    2^21 + 1 and 2^31 - 2; the sums stay within 2^61 -- T 2^B <= 2^61 for area (|q| <= 2^B), T 2^(B + 2) <= 2^61 for angle -- and the
    workspace bytes at the limits do not overflow.  The area bound is reached with equality exactly when T is a power of two of at least
    2^21 (T = 2^21: 2^21 2^40); every other T stays strictly below, and 2^61 itself is a quarter of what an int64 holds."""
    lines = run_host_program(tmp_path, 'normals_plan_main.cpp').splitlines()
    assert lines[-1] == 'bad 0'
    t_rows = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('T ')]
    v_rows = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('V ')]
    assert len(t_rows) == 14 and len(v_rows) == 14
    for T, L_, Ba, Bg, blocks in t_rows:
        assert L_ == (T - 1).bit_length()
        assert Ba == min(40, 61 - L_) == NR.term_bits(T, NR.AREA) and Bg == min(40, 59 - L_) == NR.term_bits(T, NR.ANGLE)
        assert T * 2 ** Ba <= 2 ** 61 and T * 2 ** (Bg + 2) <= 2 ** 61
        assert T * 2 ** Ba < 2 ** 61 or (T & (T - 1) == 0 and T >= 2 ** 21)
        assert blocks == -(-T // 256)
    got = {r[0]: r[2:4] for r in t_rows}
    assert got[1] == (40, 40) and got[2 ** 21] == (40, 38) and got[2 ** 21 + 1] == (39, 37) and got[T_MAX] == (30, 28)
    for V, sb, wb in v_rows:
        assert sb == -(-24 * V // 256) * 256 and wb == sb + 256
    assert (T_MAX, 24 * T_MAX + 48, 24 * T_MAX + 304) in v_rows


# ---- 4. PLY ---------------------------------------------------------------------------------------------------------------------------------
def _plain_ply_bytes(v, f):
    """the file write_ply(path, v, f) has always written"""
    faces = np.empty(len(f), dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    faces['n'] = 3
    faces['idx'] = f
    head = (f'ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n'
            f'element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n')
    return head.encode('ascii') + np.ascontiguousarray(v, '<f4').tobytes() + faces.tobytes()


def test_ply_round_trip_with_normals(tmp_path, M):
    v, f = _icosphere(1, 0.5, bumps=0.05)
    n, _ = NR.vertex_normals(v, f, 'angle')
    n[3] = [0.0, -0.0, np.float32(1e-42)]                               # a signed zero and a subnormal travel too
    plain, smooth = str(tmp_path / 'plain.ply'), str(tmp_path / 'smooth.ply')
    M.write_ply(plain, v, f)
    assert open(plain, 'rb').read() == _plain_ply_bytes(v, f)
    M.write_ply(plain, v, f, normals=None)
    assert open(plain, 'rb').read() == _plain_ply_bytes(v, f)
    M.write_ply(smooth, v, f, normals=n)
    head = open(smooth, 'rb').read().split(b'end_header\n')[0].decode()
    assert 'property float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face' in head
    v2, f2, n2 = M.read_ply(smooth, with_normals=True)
    assert np.array_equal(_bits(v2.astype(np.float32)), _bits(v)) and np.array_equal(f2, f) and n2.dtype == np.float32
    assert np.array_equal(_bits(n2), _bits(n))
    got = M.read_ply(smooth)
    assert len(got) == 2 and np.array_equal(got[0], v2) and np.array_equal(got[1], f2)       # the default return value: as it was
    v3, f3, n3 = M.read_ply(plain, with_normals=True)
    assert n3 is None and np.array_equal(v3, v2) and np.array_equal(f3, f)
    with pytest.raises(ValueError, match='normals'):
        M.write_ply(smooth, v, f, normals=n[:-1])
    # an ascii file with normals
    asc = str(tmp_path / 'ascii.ply')
    with open(asc, 'w') as fh:
        fh.write('ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n'
                 'property float ny\nproperty float nz\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n'
                 '0 0 0 0 0 1\n1 0 0 0 0 1\n0 1 0 0 0.6 0.8\n3 0 1 2\n')
    _, _, n4 = M.read_ply(asc, with_normals=True)
    assert np.array_equal(n4, np.asarray([[0, 0, 1], [0, 0, 1], [0, 0.6, 0.8]], np.float32))


# ---- 5. winding ------------------------------------------------------------------------------------------------------------------------------
def test_winding_sign(M):
    import torch
    v, f = _icosphere(2, 0.5, bumps=0.05)
    assert M.winding_sign(v, f) == 1 and M.winding_sign(v, f[:, ::-1].copy()) == -1
    assert M.winding_sign(torch.from_numpy(v) + 3.0, torch.from_numpy(f)) == 1             # the centroid is moved to the origin first
    assert M.winding_sign(v[:3], np.asarray([[0, 1, 2]], np.int32)) == 0
    tri = np.asarray([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.7, 0.9]], np.float32)
    assert M.winding_sign(tri, np.asarray([[0, 1, 2]], np.int32)) == 0                     # a sheet encloses nothing, rounding noise or not
    cv, cf = NR.cube()
    assert M.winding_sign(cv, cf) == 1
    v2, f2, _ = NR.spoiled(v, f)
    assert M.winding_sign(v2, f2) == 1                                                     # refused faces and a NaN vertex are left out
