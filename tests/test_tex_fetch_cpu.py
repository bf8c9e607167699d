"""CPU tier of the texture lookup (include/nero_hip_texfetch.h, nero_amd/csrc/tex_fetch.hip, nero_amd/texfetch.py; its binding:
tests/test_binding_cpu.py): the entry points' refusals before any device call, the restatement (tests/texfetch_ref.py) checked against
itself, and the pyramid's level arithmetic as a stand-alone program under the sanitizers."""
import numpy as np
import pytest

from tests import texfetch_ref as TR
from tests.helpers import run_host_program

ERR_ARG = -1


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib
    return _lib


# ---- 1. the surface: refusals (the binding: tests/test_binding_cpu.py) ----------------------------------------------------------------------
def test_level_counts_and_sizes_of_the_pyramid(L):
    lib = L.lib
    for (h, w), n in {(1, 1): 1, (2, 2): 2, (4, 2): 2, (6, 10): 2, (8, 8): 4, (64, 64): 7, (96, 80): 5, (1000, 1000): 4, (2048, 2048): 12,
                      (16384, 16384): 15, (16384, 3): 1}.items():
        assert lib.nero_tex_mip_levels(h, w) == n == TR.levels(h, w), (h, w)
        assert lib.nero_tex_mip_bytes(h, w) == 8 * sum((h >> k) * (w >> k) for k in range(n))
    for h, w in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-1, 8), (2 ** 40, 2 ** 40)):
        assert lib.nero_tex_mip_levels(h, w) == 0 and lib.nero_tex_mip_bytes(h, w) == 0


def test_entry_points_refuse_bad_arguments_without_a_device(L):
    lib = L.lib
    p = 4096                                                          # a non-null, aligned pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    order = {'nero_tex_pack': ('albedo', 'metallic', 'roughness', 'h', 'w', 'out', 'stream'),
             'nero_tex_mip_build': ('pyramid', 'h', 'w', 'stream'),
             'nero_tex_face_scale': ('verts', 'V', 'tris', 'vt', 'Vt', 'ft', 'T', 'h', 'w', 'scale', 'stream'),
             'nero_tex_materials': ('pyramid', 'h', 'w', 'lut', 'vt', 'Vt', 'ft', 'T', 'scale', 'face', 'bary', 'depth', 'n', 'spread', 'lod_scale',
                                    'mat5', 'dbg', 'stream'),
             'nero_tex_vertex_materials': ('pyramid', 'h', 'w', 'lut', 'vt', 'Vt', 'tris', 'ft', 'T', 'V', 'owner_ws', 'mat5_v', 'stream')}
    counts = {'V': 4, 'Vt': 4, 'T': 2, 'n': 3, 'h': 8, 'w': 8}
    floats = {'spread': 0.5, 'lod_scale': 1.0}
    required = {'nero_tex_pack': ('albedo', 'metallic', 'roughness', 'out'), 'nero_tex_mip_build': ('pyramid',),
                'nero_tex_face_scale': ('verts', 'tris', 'vt', 'ft', 'scale'),
                'nero_tex_materials': ('pyramid', 'lut', 'vt', 'ft', 'scale', 'face', 'bary', 'depth', 'mat5'),
                'nero_tex_vertex_materials': ('pyramid', 'lut', 'vt', 'tris', 'ft', 'owner_ws', 'mat5_v')}
    for name, names in order.items():
        def call(**kw):
            args = [kw[k] if k in kw else counts[k] if k in counts else floats[k] if k in floats else None if k in ('stream', 'dbg') else p for k in names]
            return getattr(lib, name)(*args)
        for h, w in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-1, 8), (8, -3), (2 ** 40, 2 ** 40)):
            assert call(h=h, w=w) == ERR_ARG and '[1, 16384]' in err() and err().startswith(name), (name, h, w)
        for k in names:
            if k in ('V', 'Vt', 'T', 'n'):
                for bad in (-1, 2 ** 31 - 1, 2 ** 40):
                    assert call(**{k: bad}) == ERR_ARG and ('2^31 - 1' in err()) and err().startswith(name), (name, k, bad)
        for k in required[name]:
            assert call(**{k: None}) == ERR_ARG and 'null pointer' in err() and err().startswith(name), (name, k)
        for k in ('pyramid', 'out'):
            if k in names:
                assert call(**{k: p + 4}) == ERR_ARG and '8-byte aligned' in err(), (name, k)
    mat = lambda **kw: lib.nero_tex_materials(*[kw[k] if k in kw else counts[k] if k in counts else floats[k] if k in floats
                                                else None if k in ('stream', 'dbg') else p for k in order['nero_tex_materials']])
    for k in ('spread', 'lod_scale'):
        for bad in (-1.0, float('nan'), -float('inf')):
            assert mat(**{k: bad}) == ERR_ARG and 'must not be negative or NaN' in err()
    assert lib.nero_tex_vertex_materials(p, 8, 8, p, p, 4, p, p, (2 ** 31 - 1) // 3, 4, p, p, None) == ERR_ARG and '(2^31 - 1) / 3' in err()
    # nothing to do: no device call either, whatever the pointers are
    assert mat(n=0, pyramid=None, mat5=None) == 0
    assert lib.nero_tex_face_scale(None, 0, None, None, 0, None, 0, 8, 8, None, None) == 0
    assert lib.nero_tex_vertex_materials(None, 8, 8, None, None, 0, None, None, 0, 0, None, None, None) == 0
    assert lib.nero_tex_mip_build(p, 1, 1, None) == 0 and lib.nero_tex_mip_build(p, 3, 16384, None) == 0      # one level: nothing is launched


def test_host_layer_and_the_table(L):
    from nero_amd import texfetch as TF
    assert np.array_equal(TF.srgb_lut().view(np.uint32), TR.srgb_lut().view(np.uint32)) and TF.srgb_lut().dtype == np.float32
    assert TF.mip_levels(1000, 1000) == 4 and TF.mip_levels(1, 1) == 1
    with pytest.raises(ValueError, match='16384'):
        TF.mip_levels(0, 4)
    import inspect
    from nero_amd.relight import Relighter
    sig = inspect.signature(Relighter.__init__).parameters
    assert sig['textures'].default is None and sig['lod_bias'].default == 0.0
    assert list(sig)[:12] == ['self', 'verts', 'tris', 'materials', 'env', 'convention', 'env_rotation', 'tracer', 'build', 'geometry_type',
                              'normals', 'device']                                   # the arguments of before, where they were
    assert inspect.signature(Relighter.surface).parameters['spread'].default is None and hasattr(Relighter, 'from_asset')


# ---- 2. the restatement against itself ------------------------------------------------------------------------------------------------------
def test_the_table_inverts_the_curve_to_within_one_byte_level():
    lut = TR.srgb_lut()
    assert lut.dtype == np.float32 and lut[0] == 0.0 and lut[255] == 1.0 and (np.diff(lut) > 0).all()
    back = np.floor(TR.linear_to_srgb(lut.astype(np.float64)) * 255.0)            # nero_tex_quantize truncates
    assert np.abs(back - np.arange(256)).max() <= 1
    s = np.arange(256) / 255.0
    assert np.array_equal(lut[:11], (s[:11] * 25.0 / 323.0).astype(np.float32)) and s[10] <= 0.04045 < s[11]      # both branches, the knee between 10 and 11


def _flat_case(n, seed=0):
    """n hits on one face that covers the whole map, footprints from below one texel to far beyond any level"""
    g = np.random.default_rng(seed)
    vt = np.asarray([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
    ft = np.asarray([[0, 1, 2], [3, 2, 1]], np.int32)
    bary = g.uniform(0, 1, (n, 2)).astype(np.float32)
    bary[:, 1] *= 1 - bary[:, 0]
    depth = np.exp2(g.uniform(-3, 12, n)).astype(np.float32)
    return dict(vt=vt, ft=ft, scale=np.asarray([1.0, 3.0], np.float32), face=g.integers(0, 2, n).astype(np.int32), bary=bary, depth=depth)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_constant_map_is_exact_at_every_level_of_detail(dtype):
    lut = TR.srgb_lut()
    c = _flat_case(500)
    for h, w in ((1, 1), (6, 10), (64, 64), (96, 80)):
        alb, met, rgh = np.empty((h, w, 3), np.uint8), np.full((h, w), 200, np.uint8), np.full((h, w), 77, np.uint8)
        alb[:] = (13, 128, 255)
        lv = TR.pyramid(alb, met, rgh)
        assert all((l[..., :5] == (13, 128, 255, 200, 77)).all() and not l[..., 5:].any() for l in lv)
        for spread, bias in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (1e30, 0.0)):
            mat5, dbg = TR.fetch(lv, lut, spread=spread, lod_scale=2.0 ** bias, dtype=dtype, **c)
            want = np.asarray([lut[200], np.sqrt(lut[77].astype(dtype)), lut[13], lut[128], lut[255]], dtype)
            assert np.array_equal(mat5, np.broadcast_to(want, mat5.shape)), (h, w, spread, bias)
            if spread == 1.0 and bias == 0.0:
                assert len(np.unique(dbg[:, 0])) == len(lv)                           # every level is visited


def test_a_texel_centre_at_unit_footprint_returns_the_decoded_byte():
    lut = TR.srgb_lut()
    h, w = 8, 16                                                                      # powers of two: every texel centre is a float32
    alb, met, rgh = TR.random_maps(h, w)
    lv = TR.pyramid(alb, met, rgh)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    vt = np.stack([(xs.reshape(-1) + 0.5) / w, (ys.reshape(-1) + 0.5) / h], -1).astype(np.float32)
    n = h * w
    ft = np.stack([np.arange(n), (np.arange(n) + 1) % n, (np.arange(n) + 2) % n], -1).astype(np.int32)
    c = dict(vt=vt, ft=ft, scale=np.ones(n, np.float32), face=np.arange(n, dtype=np.int32), bary=np.zeros((n, 2), np.float32),
             depth=np.ones(n, np.float32))
    mat5, dbg = TR.fetch(lv, lut, spread=1.0, lod_scale=1.0, **c)                     # s = 1: level 0, t = 0
    assert not dbg[:, :2].any() and not dbg[:, 4:6].any()
    assert np.array_equal(dbg[:, 2], xs.reshape(-1)) and np.array_equal(dbg[:, 3], ys.reshape(-1))
    assert np.array_equal(mat5[:, 0], lut[met.reshape(-1)]) and np.array_equal(mat5[:, 2:5], lut[alb.reshape(-1, 3)])
    assert np.array_equal(mat5[:, 1], np.sqrt(lut[rgh.reshape(-1)]))


def test_the_result_is_continuous_across_a_level_boundary():
    """s = 2 - 2^-20 (level 0, t = 1 - 2^-20) against s = 2 (level 1, t = 0): the values differ by no more than 2^-20 of the largest
    difference between two levels (1: bytes decode into [0, 1]) and the rounding of the mix -- and the square root's slope on the
    roughness, so that column is compared squared"""
    lut = TR.srgb_lut()
    lv = TR.pyramid(*TR.random_maps(64, 64))
    c = _flat_case(400, seed=3)
    c['scale'][:] = 1.0
    below, above = dict(c, depth=np.full(400, 2.0 - 2.0 ** -20, np.float32)), dict(c, depth=np.full(400, 2.0, np.float32))
    a, da = TR.fetch(lv, lut, spread=1.0, lod_scale=1.0, dtype=np.float64, **below)
    b, db = TR.fetch(lv, lut, spread=1.0, lod_scale=1.0, dtype=np.float64, **above)
    assert (da[:, 0] == 0).all() and (da[:, 1] == 1.0 - 2.0 ** -20).all() and (db[:, 0] == 1).all() and not db[:, 1].any()
    a[:, 1], b[:, 1] = a[:, 1] ** 2, b[:, 1] ** 2
    assert np.abs(a - b).max() <= 2.0 ** -20 + 1e-12
    a32 = TR.fetch(lv, lut, spread=1.0, lod_scale=1.0, dtype=np.float32, **below)[0]
    b32 = TR.fetch(lv, lut, spread=1.0, lod_scale=1.0, dtype=np.float32, **above)[0]
    a32[:, 1], b32[:, 1] = a32[:, 1] ** 2, b32[:, 1] ** 2
    assert np.abs(a32.astype(np.float64) - b32).max() <= 2.0 ** -20 + 8 * 2.0 ** -24  # ... and a few float32 roundings of values below 1
    # monotone in s: the level and then t never fall as the footprint grows
    depth = np.sort(np.exp2(np.random.default_rng(5).uniform(-2, 9, 400))).astype(np.float32)
    _, l, t = TR.lod(depth, 1.0, np.ones(400, np.float32), 1.0, len(lv))
    key = l + t.astype(np.float64)
    assert (np.diff(key) >= 0).all() and l.max() == len(lv) - 1 and l.min() == 0


def test_the_recorded_floor_is_what_the_shared_inputs_measure():
    """F32_FLOOR, the basis of the GPU tier's tolerance, is the float32 restatement against the float64 one over the GPU tier's own inputs"""
    got = TR.measure_floor()
    print(f'float32 against float64 over fetch_cases(): {got:.4e} (recorded {TR.F32_FLOOR:.4e}, GPU bound {TR.GPU_FACTOR * TR.F32_FLOOR:.4e})')
    assert 0.9 * TR.F32_FLOOR <= got <= TR.F32_FLOOR and TR.GPU_FACTOR == 4.0


def test_special_lanes_of_the_restatement():
    lut = TR.srgb_lut()
    lv = TR.pyramid(*TR.random_maps(6, 10))
    c = TR.fetch_case(6, 10, 65)
    k = len(TR.SPECIAL_UV)
    for spread, bias in TR.LODS:
        mat5, dbg = TR.fetch(lv, lut, spread=spread, lod_scale=2.0 ** bias, **c)
        assert np.isfinite(mat5).all() and (mat5 >= 0).all() and (mat5 <= 1).all()
        assert not mat5[k:k + 4].any() and not dbg[k:k + 4].any()                     # a miss, face == T, two bad UV indices
        assert mat5[:k].any(1).all()                                                  # a coordinate that is not finite reads some texel
        assert (dbg[:, 2] >= -1).all() and (dbg[:, 2] <= 10).all() and (dbg[:, 3] >= -1).all() and (dbg[:, 3] <= 6).all()
        if spread == 0.0:
            assert not dbg[:, :2].any()
        if spread >= 1e30:
            live = np.ones(65, bool)
            live[k:k + 4] = False
            pinned = live & (c['scale'][np.clip(c['face'], 0, TR.T_FACES - 1)] > 0)
            assert (dbg[pinned, 0] == len(lv) - 1).all() and not dbg[:, 1].any()


def test_vertex_owners_of_the_restatement():
    tris = np.asarray([[2, 1, 0], [0, 1, 3], [5, 9, 1]], np.int32)                    # vertex 4 is named by nobody, 9 is out of range (V = 6)
    ft = np.asarray([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    vt = np.random.default_rng(1).uniform(0, 1, (9, 2)).astype(np.float32)
    lv = TR.pyramid(*TR.random_maps(8, 8))
    mat5, owner = TR.vertex_materials(lv, TR.srgb_lut(), vt, tris, ft, 6)
    assert owner.tolist() == [2, 1, 0, 5, TR.NO_OWNER, 6]
    assert not mat5[4].any() and mat5[[0, 1, 2, 3, 5]].any(1).all()
    want = TR._mat5(TR.bilinear(lv[0], TR.srgb_lut(), vt[[2, 1, 0, 5, 6], 0], vt[[2, 1, 0, 5, 6], 1])[0])
    assert np.array_equal(mat5[[0, 1, 2, 3, 5]], want)


# ---- 3. levels and offsets ------------------------------------------------------------------------------------------------------------------
def test_pyramid_arithmetic_under_the_sanitizers(tmp_path):
    """nero_amd/csrc/tex_fetch_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program): the level counts and
    offsets tile the pyramid without gap or overlap at 1 x 1, 2 x 2, 4 x 2, 6 x 10, 1000 x 1000, 16384 x 16384 and the GPU tier's other
    sizes; the argument checks hold at their edges"""
    lines = run_host_program(tmp_path, 'tex_fetch_plan_main.cpp').splitlines()
    assert lines[-1] == 'bad 0'
    rows = {(r[0], r[1]): r[2:] for r in (tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('P '))}
    assert len(rows) == 12
    for (h, w), (L_, records, nbytes) in rows.items():
        assert L_ == TR.levels(h, w) and records == sum((h >> k) * (w >> k) for k in range(L_)) and nbytes == 8 * records
    assert rows[(1, 1)] == (1, 1, 8) and rows[(2, 2)] == (2, 5, 40) and rows[(4, 2)] == (2, 10, 80) and rows[(6, 10)] == (2, 75, 600)
    assert rows[(1000, 1000)][0] == 4 and rows[(16384, 16384)][0] == 15 and rows[(16384, 16384)][1] == (4 ** 15 - 1) // 3
    lv = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('V ')]
    assert [r[2:] for r in lv if r[:2] == (1000, 1000)] == [(0, 1000, 1000, 0), (1, 500, 500, 1000000), (2, 250, 250, 1250000), (3, 125, 125, 1312500)]
