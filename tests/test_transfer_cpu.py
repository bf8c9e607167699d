"""CPU tier of detail transfer (include/nero_transfer.h, nero_amd/csrc/detail_transfer.hip, nero_amd/transfer.py): the binding from the
third header list, the entry points' refusals before any device call, the restatement (tests/transfer_ref.py) checked against itself and
against the conventions the header states, and the textured OBJ with and without a normal map."""
import inspect
import os

import numpy as np
import pytest

from tests import transfer_ref as R

ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib
    return _lib


ENTRY_POINTS = {'nero_mesh_attr_at', 'nero_uv_tangents_workspace_bytes', 'nero_uv_tangents', 'nero_nmap_encode', 'nero_nmap_mip_bytes', 'nero_nmap_pack',
                'nero_nmap_mip_build', 'nero_nmap_apply'}


# ---- 1. the binding ---------------------------------------------------------------------------------------------------------------------------
def test_the_header_is_bound_from_the_third_list(L):
    import ctypes as C
    assert [os.path.basename(p) for p in L.NEWER_HEADER_PATHS] == ['nero_transfer.h']
    assert not set(L.NEWER_HEADER_PATHS) & (set(L.HEADER_PATHS) | set(L.EXTRA_HEADER_PATHS))
    sigs = L.parse_headers(L.NEWER_HEADER_PATHS)
    assert set(sigs) == ENTRY_POINTS
    assert not set(sigs) & (set(L.parse_headers()) | set(L.parse_headers(L.EXTRA_HEADER_PATHS)))
    for fn, (restype, argtypes, header) in sigs.items():
        f = getattr(L.lib, fn)
        assert f.restype is restype and list(f.argtypes) == argtypes and header == 'nero_transfer.h', fn
    assert L.lib.nero_nmap_apply.argtypes[1] is C.c_int64 and L.lib.nero_nmap_apply.argtypes[15] is C.c_float
    assert L.lib.nero_nmap_mip_bytes.restype is C.c_size_t and L.lib.nero_mesh_attr_at.argtypes[2] is C.c_int
    assert 'NEWER_HEADER_PATHS' in inspect.getsource(L._load)


def test_a_newer_header_makes_the_library_stale(L):
    import __graft_entry__ as ge
    path = L.NEWER_HEADER_PATHS[0]
    assert path in ge._sources()[1] and os.path.join(ROOT, 'nero_amd', 'csrc', 'detail_transfer.hip') in ge._sources()[0]
    assert not ge.library_is_stale()
    st = os.stat(path)
    try:
        os.utime(path, (st.st_atime, os.path.getmtime(ge.LIB) + 10))
        assert ge.library_is_stale()
    finally:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not ge.library_is_stale()


# ---- 2. refusals, before any device call ------------------------------------------------------------------------------------------------------
ORDER = {'nero_mesh_attr_at': ('attr', 'V', 'C', 'tris', 'T', 'face', 'bary', 'n', 'fill', 'out', 'stream'),
         'nero_uv_tangents': ('verts', 'V', 'tris', 'vt', 'Vt', 'ft', 'T', 'ws', 'tangent', 'face_sign', 'info', 'stream'),
         'nero_nmap_encode': ('nrm', 'tan', 'sign', 'ns', 'valid', 'texel', 'n', 'h', 'w', 'space', 'map', 'invalid', 'stream'),
         'nero_nmap_pack': ('map', 'h', 'w', 'out', 'stream'),
         'nero_nmap_mip_build': ('pyramid', 'h', 'w', 'stream'),
         'nero_nmap_apply': ('pyramid', 'h', 'w', 'vt', 'Vt', 'ft', 'T', 'scale', 'tangent', 'face_sign', 'face', 'bary', 'depth', 'nrm_in', 'n', 'spread',
                             'lod_scale', 'space', 'nrm_out', 'dbg', 'stream')}
SCALARS = {'V': 4, 'Vt': 4, 'T': 2, 'n': 3, 'h': 8, 'w': 8, 'C': 3, 'space': 0, 'spread': 0.5, 'lod_scale': 1.0, 'fill': 0.0}
OPTIONAL = ('stream', 'dbg')


def _caller(lib, name):
    p = 4096                                                          # non-null, aligned, never followed: every call below is refused first
    def call(**kw):
        return getattr(lib, name)(*[kw[k] if k in kw else SCALARS[k] if k in SCALARS else None if k in OPTIONAL else p for k in ORDER[name]])
    return call


def test_entry_points_refuse_bad_arguments_without_a_device(L):
    lib = L.lib
    err = lambda: lib.nero_last_error().decode()
    assert set(ORDER) | {'nero_uv_tangents_workspace_bytes', 'nero_nmap_mip_bytes'} == ENTRY_POINTS
    for name, names in ORDER.items():
        call = _caller(lib, name)
        if 'h' in names:
            for h, w in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-1, 8), (8, -3), (2 ** 40, 2 ** 40)):
                assert call(h=h, w=w) == ERR_ARG and '[1, 16384]' in err() and err().startswith(name), (name, h, w)
        for k in names:
            if k in ('V', 'Vt', 'T', 'n'):
                for bad in (-1, 2 ** 31 - 1, 2 ** 40):
                    assert call(**{k: bad}) == ERR_ARG and '2^31 - 1' in err() and err().startswith(name), (name, k, bad)
            elif k not in SCALARS and k not in OPTIONAL:
                assert call(**{k: None}) == ERR_ARG and 'null pointer' in err() and err().startswith(name), (name, k)
        if 'space' in names:
            for bad in (-1, 2, 7):
                assert call(space=bad) == ERR_ARG and 'space must be 0' in err(), (name, bad)
    for bad in (0, 9, -1, 64):
        assert _caller(lib, 'nero_mesh_attr_at')(C=bad) == ERR_ARG and '[1, 8]' in err()
    for k in ('spread', 'lod_scale'):
        for bad in (-1.0, float('nan'), -float('inf')):
            assert _caller(lib, 'nero_nmap_apply')(**{k: bad}) == ERR_ARG and 'must not be negative or NaN' in err()
    assert _caller(lib, 'nero_nmap_apply')(pyramid=4098) == ERR_ARG and '4-byte aligned' in err()
    assert _caller(lib, 'nero_nmap_pack')(out=4097) == ERR_ARG and _caller(lib, 'nero_nmap_mip_build')(pyramid=4102) == ERR_ARG
    assert _caller(lib, 'nero_uv_tangents')(ws=4096 + 128) == ERR_ARG and '256-byte aligned' in err()
    # nothing to do: no device call either, whatever the pointers are
    assert lib.nero_mesh_attr_at(None, 0, 1, None, 0, None, None, 0, 0.0, None, None) == 0
    assert _caller(lib, 'nero_nmap_apply')(n=0, pyramid=None, nrm_out=None) == 0
    assert _caller(lib, 'nero_nmap_encode')(n=0, map=None, invalid=None) == 0
    assert _caller(lib, 'nero_uv_tangents')(T=0, ws=None) == 0 and _caller(lib, 'nero_uv_tangents')(Vt=0, tangent=None) == 0
    assert lib.nero_nmap_mip_build(4096, 1, 1, None) == 0 and lib.nero_nmap_mip_build(4096, 3, 16384, None) == 0   # one level: nothing is launched


def test_sizes_of_the_pyramid_and_the_workspace(L):
    lib = L.lib
    for (h, w), n in {(1, 1): 1, (2, 2): 2, (6, 10): 2, (64, 64): 7, (96, 80): 5, (1000, 1000): 4, (16384, 16384): 15}.items():
        assert lib.nero_tex_mip_levels(h, w) == n
        assert lib.nero_nmap_mip_bytes(h, w) == 4 * sum((h >> k) * (w >> k) for k in range(n)) == lib.nero_tex_mip_bytes(h, w) // 2
    for h, w in ((0, 8), (8, 16385), (-1, 8)):
        assert lib.nero_nmap_mip_bytes(h, w) == 0
    for Vt in (1, 10, 11, 1000):
        assert lib.nero_uv_tangents_workspace_bytes(Vt, 5) == 256 + (24 * Vt + 255) // 256 * 256
    assert lib.nero_uv_tangents_workspace_bytes(-1, 5) == 0 and lib.nero_uv_tangents_workspace_bytes(5, 2 ** 31 - 1) == 0
    assert [R.term_bits(T) for T in (1, 2, 3, 2 ** 20, 2 ** 21, 2 ** 21 + 1, 2 ** 31 - 2)] == [40, 40, 40, 40, 40, 39, 30]


def test_host_layer(L):
    from nero_amd import transfer as TF
    from nero_amd.relight import Relighter
    sig = inspect.signature(Relighter.__init__).parameters
    assert sig['normal_map'].default is None and list(sig)[-1] == 'normal_map' and list(sig)[-3:-1] == ['textures', 'lod_bias']
    s = inspect.signature(TF.bake_normal_map).parameters
    assert [s[k].default for k in ('size', 'ssaa', 'pad', 'border', 'space', 'normals', 'source_normals', 'max_dist', 'atlas')] == \
        [1024, 2, 32, 3, 'tangent', 'angle', 'angle', None, 'triangles']
    assert inspect.signature(TF.bake_asset).parameters['atlas'].default == 'charts'
    with pytest.raises(ValueError, match='tangent'):
        TF._space('world')
    assert TF.FLAT == R.FLAT == (128, 128, 255)


# ---- 3. the restatement -----------------------------------------------------------------------------------------------------------------------
def test_bytes_round_trip_within_half_a_level():
    """decode(encode(x)) is within 1 / 254 per component: rounding 127 x to the nearest integer moves it by at most 1/2, and the clamp at 1
    only touches x below -1 + 1/254.  That bound is asserted as it stands on the float64 restatement, where it is attainable.  The float32
    restatement rounds x (half an ulp of a value up to 1: 2^-25) and 127 x (half an ulp of a value below 128: 2^-18) before it rounds to an
    integer, so it sees 127 x moved by at most 127 * 2^-25 + 2^-18 < 2^-17: its bytes are the float64 bytes except where 127 x lies within
    2^-17 of a half-integer, and there they are the neighbouring level (measured: float32 reaches 0.003937035 against 1/254 =
    0.003937008 at such a tie, so 1/254 itself is not a float32 property)."""
    g = np.random.default_rng(0)
    x = g.normal(size=(100000, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    b64 = R.to_bytes(x)
    assert b64.min() >= 1 and np.abs(R.decode(b64, np.float64) - x).max() <= 1.0 / 254.0
    x32 = x.astype(np.float32)
    b32 = R.to_bytes(x32)
    err32 = np.abs(R.decode(b32, np.float32).astype(np.float64) - x).max()
    print(f'decode(encode(x)): float64 {np.abs(R.decode(b64, np.float64) - x).max():.9f}, float32 {err32:.9f}, 1/254 = {1 / 254:.9f}')
    differ = b32 != b64
    tie = np.abs(np.abs(127.0 * x - np.floor(127.0 * x)) - 0.5) <= 2.0 ** -17
    assert not (differ & ~tie).any() and np.abs(b32.astype(np.int32) - b64.astype(np.int32)).max() <= 1
    assert R.to_bytes(np.asarray([[0, 0, 1], [0, 0, -1], [1, -1, 0]], np.float32)).tolist() == [[128, 128, 255], [128, 128, 1], [255, 1, 128]]
    assert R.decode(np.asarray([128, 255, 1]), np.float32).tolist() == [0.0, 1.0, -1.0]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_flat_normal_and_the_flat_pyramid(dtype):
    g = np.random.default_rng(1)
    N = g.normal(size=(500, 3)) * np.exp2(g.uniform(-20, 3, (500, 1)))                # any length
    T = g.normal(size=(500, 3))
    T[:20] = 0                                                                        # no tangent: the fallback axis
    T[20:40] = N[20:40] * 3                                                           # parallel to the normal: likewise
    sign = g.integers(-1, 2, 500).astype(np.int8)
    by, bad = R.encode(N, T, sign, N, np.ones(500, np.uint8), R.TANGENT, dtype)
    assert (by == R.FLAT).all() and not bad.any()                                     # the source normal IS the frame normal: flat
    n, t, b, ln, ok = R.frame(N, T, sign, dtype)
    assert ok.all() and np.abs(R.dot3(n, t)).max() < 1e-5 and np.abs(R.dot3(n, b)).max() < 1e-5 and np.abs(R.dot3(t, b)).max() < 1e-5
    assert np.abs(R.dot3(t, t) - 1).max() < 1e-5 and np.abs(R.dot3(b, b) - 1).max() < 1e-5
    hand = R.dot3(np.cross(n, t), b)
    assert ((hand > 0) == (sign >= 0)).all()
    nmap = np.empty((96, 80, 3), np.uint8)
    nmap[:] = R.FLAT
    lv = R.pyramid(nmap)
    assert len(lv) == 5 and all((l[..., :3] == R.FLAT).all() and not l[..., 3].any() for l in lv)
    # invalid texels: the flat value in tangent space, the frame normal's bytes in object space, and they are counted
    ns = N.copy()
    ns[:5], ns[5:10] = 0, np.nan
    valid = np.ones(500, np.uint8)
    valid[10:15] = 0
    by, bad = R.encode(N, T, sign, ns, valid, R.TANGENT, dtype)
    assert bad.sum() == 15 and bad[:15].all() and (by == R.FLAT).all()
    by, bad = R.encode(N, T, sign, ns, valid, R.OBJECT, dtype)
    assert bad.sum() == 15 and np.array_equal(by, R.to_bytes(R.unit3(N.astype(dtype))[0]))


@pytest.mark.parametrize('mirror', [False, True])
def test_the_bitangent_points_along_the_files_v(mirror):
    """the unit square with u = x (mirror: u runs along -x) and FILE v = y: T = +x (-x), B = +y either way, face_sign +1 (-1)"""
    verts, tris, vt, ft = R.unit_square(mirror)
    tangent, sign, info = R.uv_tangents(verts, tris, vt, ft)
    sx = -1.0 if mirror else 1.0
    assert np.array_equal(tangent, np.tile(np.asarray([[sx, 0, 0]], np.float32), (4, 1)))
    assert sign.tolist() == ([-1, -1] if mirror else [1, 1]) and info.tolist() == [0, 0, 0, 1]
    for dtype in (np.float32, np.float64):
        n, t, b, _, ok = R.frame(np.tile([[0.0, 0.0, 2.0]], (4, 1)), tangent, np.full(4, sign[0]), dtype)
        assert ok.all() and np.array_equal(n, np.tile([[0, 0, 1]], (4, 1))) and np.array_equal(t, np.tile([[sx, 0, 0]], (4, 1)))
        assert np.array_equal(b, np.tile([[0, 1, 0]], (4, 1)))
        # a source normal leaning towards +y (up in the file) is GREEN above 128 whichever way u runs; towards +x it is red above 128
        # only where u runs along +x
        by, bad = R.encode(np.tile([[0, 0, 1.0]], (2, 1)), tangent[:2], np.full(2, sign[0]), np.asarray([[0, 0.6, 0.8], [0.6, 0, 0.8]]),
                           np.ones(2), R.TANGENT, dtype)
        assert not bad.any() and by[0].tolist() == [128, 204, 230] and by[1].tolist() == [128 + int(sx) * 76, 128, 230]


def test_tangents_of_the_restatement():
    """degenerate and refused faces contribute nothing and are counted; the sums do not depend on the order of the faces"""
    from nero_amd.synthetic import icosphere
    from nero_amd.texture import simple_atlas
    v, f = icosphere(2)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int32)
    vt, ft = simple_atlas(v, f, 128)
    tangent, sign, info = R.uv_tangents(v, f, vt, ft)
    assert info[:3].tolist() == [0, 0, 0] and (np.abs(sign) == 1).all() and np.abs(np.linalg.norm(tangent, axis=1) - 1).max() < 1e-6
    perm = np.random.default_rng(3).permutation(len(f))
    t2, s2, i2 = R.uv_tangents(v, f[perm], vt, ft[perm])
    assert np.array_equal(t2.view(np.uint32), tangent.view(np.uint32)) and np.array_equal(s2, sign[perm]) and np.array_equal(i2, info)
    ft_bad, f_bad = ft.copy(), f.copy()
    ft_bad[0, 1] = ft_bad[0, 0]                                                       # a repeated UV index: det == 0
    ft_bad[1, 2] = len(vt)                                                            # out of range
    f_bad[2, 0] = -1
    t3, s3, i3 = R.uv_tangents(v, f_bad, vt, ft_bad)
    assert i3[:2].tolist() == [2, 1] and s3[:3].tolist() == [0, 0, 0] and np.array_equal(s3[3:], sign[3:])
    touched = np.unique(np.concatenate([ft[0], ft[1], ft[2]]))
    rest = np.setdiff1d(np.arange(len(vt)), touched)
    assert np.array_equal(t3[rest].view(np.uint32), tangent[rest].view(np.uint32)) and not t3[touched].any() and i3[2] == len(touched)


def test_attr_at_and_apply_of_the_restatement():
    g = np.random.default_rng(5)
    attr = g.normal(size=(6, 4)).astype(np.float32)
    tris = np.asarray([[0, 1, 2], [2, 3, 9], [3, 4, 5]], np.int32)                    # face 1 names vertex 9 of 6
    face = np.asarray([0, 0, 0, 2, -1, 3, 1], np.int32)
    bary = np.asarray([[0, 0], [1, 0], [0, 1], [0.25, 0.5], [0.1, 0.1], [0.1, 0.1], [0.1, 0.1]], np.float32)
    out = R.attr_at(attr, tris, face, bary, fill=-7.0)
    assert np.array_equal(out[0], attr[0]) and np.array_equal(out[4:], np.full((3, 4), -7.0, np.float32))
    assert np.abs(out[1] - attr[1]).max() <= 2.0 ** -20 and np.abs(out[2] - attr[2]).max() <= 2.0 ** -20      # two roundings of values below 8
    assert np.allclose(out[3], 0.25 * attr[3] + 0.25 * attr[4] + 0.5 * attr[5], atol=1e-6)
    # the lookup: a flat map gives nrm_in back bit for bit at every level, a constant map the same vector at every level
    verts, tris, vt, ft = R.unit_square()
    tangent, sign, _ = R.uv_tangents(verts, tris, vt, ft)
    n = 300
    face = g.integers(-1, 3, n).astype(np.int32)
    bary = g.uniform(0, 1, (n, 2)).astype(np.float32)
    bary[:, 1] *= 1 - bary[:, 0]
    depth = np.exp2(g.uniform(-3, 9, n)).astype(np.float32)
    nin = (g.normal(size=(n, 3)) * np.exp2(g.uniform(-12, 2, (n, 1)))).astype(np.float32)
    nin[:, 2] = np.abs(nin[:, 2]) + np.abs(nin[:, 0]) + np.abs(nin[:, 1])             # within 45 degrees of +z: no map below tilts it past 90
    flat = np.empty((64, 64, 3), np.uint8)
    flat[:] = R.FLAT
    const = np.empty((64, 64, 3), np.uint8)
    const[:] = (160, 100, 230)
    for dtype in (np.float32, np.float64):
        for spread in (0.0, 1.0, 1e30):
            out, dbg = R.apply(R.pyramid(flat), vt, ft, np.ones(2, np.float32), tangent, sign, face, bary, depth, nin, spread, 1.0, R.TANGENT, dtype)
            assert np.array_equal(out, nin.astype(dtype))
            oc, _ = R.apply(R.pyramid(const), vt, ft, np.ones(2, np.float32), tangent, sign, face, bary, depth, nin, spread, 1.0, R.OBJECT, dtype)
            hit = (face >= 0) & (face < 2)
            want = R.decode(np.asarray([160, 100, 230]), dtype)
            assert np.array_equal(oc[hit], np.broadcast_to(want, (hit.sum(), 3))) and np.array_equal(oc[~hit], nin[~hit].astype(dtype))
            if spread == 1.0:
                assert len(np.unique(dbg[hit, 0])) == 7
    # a map that tilts by more than a right angle: the fallback returns nrm_in
    back = np.empty((8, 8, 3), np.uint8)
    back[:] = (128, 255, 100)                                                         # z below zero
    out, _ = R.apply(R.pyramid(back), vt, ft, np.ones(2, np.float32), tangent, sign, face, bary, depth, nin, 0.0, 1.0)
    assert np.array_equal(out, nin)


# ---- 4. the textured OBJ ----------------------------------------------------------------------------------------------------------------------
def _asset():
    from nero_amd.synthetic import icosphere
    from nero_amd.texture import simple_atlas
    v, f = icosphere(1)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int32)
    vt, ft = simple_atlas(v, f, 32)
    g = np.random.default_rng(11)
    maps = {'albedo': g.integers(0, 256, (32, 32, 3), dtype=np.uint8), 'metallic': g.integers(0, 256, (32, 32), dtype=np.uint8),
            'roughness': g.integers(0, 256, (32, 32), dtype=np.uint8)}
    return v, f, vt, ft, maps, g.integers(1, 256, (32, 32, 3), dtype=np.uint8)


def _files(d):
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize('with_ao', [False, True])
def test_the_obj_without_a_normal_map_is_what_it_was_and_with_one_round_trips(L, tmp_path, with_ao):
    from nero_amd import texture as TX
    v, f, vt, ft, maps, normal = _asset()
    if with_ao:
        maps['ao'] = normal[..., 0].copy()
    plain, extra = str(tmp_path / 'plain'), str(tmp_path / 'extra')
    TX.write_textured_obj(plain, v, f, vt, ft, maps, name='mesh_3', use_pil=False)
    # 'space' and 'normals' alone (a bake_normal_map result stripped of its map) change nothing: the same path as before
    TX.write_textured_obj(extra, v, f, vt, ft, {**maps, 'space': 'object', 'normals': 'area'}, name='mesh_3', use_pil=False)
    base = _files(plain)
    assert base == _files(extra) and set(base) == {'mesh_3.obj', 'mesh_3.mtl', 'feat0_3.png', 'feat1_3.png', 'feat2_3.png'} | ({'feat3_3.png'} if with_ao else set())
    mtl = 'newmtl defaultMat\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nTr 1\nillum 1\nNs 0\nmap_Kd feat0_3.png\n' + ('map_Ka feat3_3.png\n' if with_ao else '')
    assert base['mesh_3.mtl'] == mtl.encode()                                          # the MTL of the parent commit, written out
    # the OBJ: the SHA-256 of what the writer of the commit before this feature produced for these inputs (the PNGs are pinned by content,
    # not by hash: their bytes depend on the zlib at hand)
    import hashlib
    assert hashlib.sha256(base['mesh_3.obj']).hexdigest() == 'a27adcf1aad3d8a77bc0d2d393d29f82c375fec1cc29a01536b4c1b36a3bbdfd'
    assert base['mesh_3.obj'].startswith(b'mtllib mesh_3.mtl\nv ') and base['mesh_3.obj'].count(b'\nf ') == len(f)
    for k, key in enumerate(('albedo', 'metallic', 'roughness') + (('ao',) if with_ao else ())):
        img = TX.read_png(os.path.join(plain, f'feat{k}_3.png'))
        assert img.shape == (32, 32, 3) and np.array_equal(img if k == 0 else img[..., 0], maps[key]) and (k == 0 or (img == img[..., :1]).all())
    back = TX.read_textured_obj(os.path.join(plain, 'mesh_3.obj'))
    assert not {'norm', 'normal', 'normal_space', 'normal_frame'} & set(back)
    for space, frame in (('tangent', 'angle'), ('object', 'area'), ('tangent', 'custom')):
        d = str(tmp_path / f'{space}_{frame}')
        obj = TX.write_textured_obj(d, v, f, vt, ft, {**maps, 'normal': normal, 'space': space, 'normals': frame}, name='mesh_3', use_pil=False)
        got = _files(d)
        assert {k: got[k] for k in base if k != 'mesh_3.mtl'} == {k: base[k] for k in base if k != 'mesh_3.mtl'}
        assert set(got) == set(base) | {'feat4_3.png'}
        assert got['mesh_3.mtl'] == base['mesh_3.mtl'] + f'norm feat4_3.png\n# nero_normal_map space={space} normals={frame}\n'.encode()
        back = TX.read_textured_obj(obj)
        assert back['norm'] == 'feat4_3.png' and back['normal_space'] == space and back['normal_frame'] == frame
        assert np.array_equal(back['normal'], normal) and np.array_equal(back['albedo'], maps['albedo'])
        assert 'normal' not in TX.read_textured_obj(obj, load_maps=False)
    with pytest.raises(ValueError, match='space'):
        TX.write_textured_obj(str(tmp_path / 'bad'), v, f, vt, ft, {**maps, 'normal': normal, 'space': 'world'}, name='mesh_3', use_pil=False)
