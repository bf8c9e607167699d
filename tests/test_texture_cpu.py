"""CPU tier of the texture baking (nero_amd/texture.py, nero_amd/csrc/texture.hip): the numpy restatement tests/texture_ref.py against what scipy and
sklearn -- the packages the reference calls for the gutter -- recorded in tests/golden/texture_regions.npz (scripts/gen_golden_texture.py), the
coverage rule's exact single cover, the built-in atlas, and the OBJ / PNG round trip.  No GPU, no scipy, no sklearn."""
import os

import numpy as np
import pytest

from tests import texture_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'texture_regions.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize('m', range(len(R.GUTTER_MASKS)))
@pytest.mark.parametrize('pad', R.GUTTER_PADS)
def test_ref_regions_equal_scipy(gold, m, pad):
    h, w, seed = R.GUTTER_MASKS[m]
    mask = R.gutter_mask(h, w, seed)
    assert np.array_equal(mask.astype(np.uint8), gold[f'mask_{m}'])              # the fixture belongs to these masks
    assert np.array_equal(R.regions(mask, pad, 3), gold[f'region_{m}_{pad}'])


@pytest.mark.parametrize('m', range(len(R.GUTTER_MASKS)))
@pytest.mark.parametrize('pad', R.GUTTER_PADS)
def test_ref_fill_equals_sklearn(gold, m, pad):
    """distances exactly (as squared integers); sources wherever the nearest texel is unique (sklearn leaves ties unspecified)"""
    region = gold[f'region_{m}_{pad}']
    h, w = region.shape
    tex = np.arange(h * w, dtype=np.int64).reshape(h, w, 1) % 251
    _, src, d2, ties = R.fill(tex.astype(np.uint8), region, pad, details=True)
    assert np.array_equal(d2, gold[f'd2_{m}_{pad}'].astype(np.int64))
    assert d2.max() <= pad * pad                                                    # the window argument: never farther than pad
    unique = ties == 1
    tied = 1.0 - unique.mean()
    print(f'mask {m} pad {pad}: {len(d2)} fill texels, {100 * tied:.2f} % tied, largest distance {np.sqrt(d2.max()):.1f}')
    assert tied <= 0.05
    mine = src[region == 3]
    assert np.array_equal(mine[unique], gold[f'src_{m}_{pad}'][unique])
    # on tied texels: sklearn's choice is one of the equally near search texels
    sk = gold[f'src_{m}_{pad}'][~unique].astype(np.int64)
    fy, fx = np.nonzero(region == 3)
    dd = (sk // w - fy[~unique]) ** 2 + (sk % w - fx[~unique]) ** 2
    assert np.array_equal(dd, d2[~unique]) and np.all(mine[~unique] <= sk)


@pytest.mark.parametrize('h,w,nx,ny,seed', R.GRID_CASES)
def test_raster_rule_covers_a_triangulation_exactly_once(h, w, nx, ny, seed):
    vt, ft = R.jittered_grid(h, w, nx, ny, seed)
    tri_id, cover = R.raster(vt, ft, h, w, count=True)
    assert np.array_equal(cover, np.ones((h, w), np.int32))
    assert tri_id.min() >= 0
    # mixed windings were really generated, and some vertices really sit on texel centres
    S = R.snap(vt, h, w)
    signs = {np.sign((S[f[1], 0] - S[f[0], 0]) * (S[f[2], 1] - S[f[0], 1]) - (S[f[2], 0] - S[f[0], 0]) * (S[f[1], 1] - S[f[0], 1])) for f in ft}
    assert signs == {-1.0, 1.0}
    assert np.any(np.all(S % 256 == 128, axis=1))


def test_raster_rule_special_cases():
    for name, (vt, ft, h, w, expect) in R.special_cases().items():
        tri_id, cover = R.raster(vt, ft, h, w, count=True)
        if expect == 'single':
            assert np.array_equal(cover, np.ones((h, w), np.int32)), name
        elif expect == 'empty':
            assert cover.sum() == 0 and (tri_id == -1).all(), name
        else:                                                       # triangle 0 lies over triangles 1 and 2, which tile the square
            assert cover.max() == 2 and cover.min() == 1, name
            solo = R.raster(vt, ft[:1], h, w)
            assert (solo == 0).sum() > 10 and np.array_equal(tri_id == 0, solo == 0), name
    # the shared diagonal really runs through texel centres: both triangles see e == 0 there
    vt, ft, h, w, _ = R.special_cases()['diagonal_through_centres']
    S = R.snap(vt, h, w)
    tri = R.triangle(S, ft[0])
    e, _ = R.edges_at(tri, np.int64(256 * 3 + 128), np.int64(256 * 3 + 128))
    assert 0 in [int(v) for v in e]


def test_simple_atlas_on_the_icosphere():
    from nero_amd.texture import simple_atlas
    from tests.helpers import golden_mesh
    v, f = golden_mesh()
    assert f.shape[0] == 1280
    vt, ft = simple_atlas(v, f, 256)
    assert vt.dtype == np.float32 and ft.dtype == np.int32 and ft.shape == (1280, 3) and vt.min() >= 0 and vt.max() <= 1
    tri_id, cover = R.raster(vt, ft, 256, 256, count=True)
    assert cover.max() == 1                                                        # no texel claimed by two triangles
    assert np.array_equal(np.unique(tri_id[tri_id >= 0]), np.arange(1280))          # every triangle covers at least one texel
    # charts at least two texels apart: the 8 neighbours of a covered texel hold its own chart or nothing
    padded = np.pad(tri_id, 1, constant_values=-1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nb = padded[1 + dy:257 + dy, 1 + dx:257 + dx]
            assert not np.any((tri_id >= 0) & (nb >= 0) & (nb != tri_id)), (dy, dx)
    with pytest.raises(ValueError, match='104'):                                   # 26 x 26 cells of 4 texels
        simple_atlas(v, f, 103)
    vt4, ft4 = simple_atlas(v, f, 104)                                             # the smallest size still satisfies all three properties
    t4, c4 = R.raster(vt4, ft4, 104, 104, count=True)
    assert c4.max() == 1 and np.array_equal(np.unique(t4[t4 >= 0]), np.arange(1280))
    p4 = np.pad(t4, 1, constant_values=-1)
    assert not any(np.any((t4 >= 0) & (p4[1 + dy:105 + dy, 1 + dx:105 + dx] >= 0) & (p4[1 + dy:105 + dy, 1 + dx:105 + dx] != t4))
                   for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _have_pil():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def test_textured_obj_round_trip(tmp_path):
    from nero_amd import texture as TX
    from tests.helpers import golden_mesh
    v, f = golden_mesh()
    vt, ft = TX.simple_atlas(v, f, 128)
    rng = np.random.default_rng(5)
    maps = {'albedo': rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), 'metallic': rng.integers(0, 256, (24, 40), dtype=np.uint8),
            'roughness': rng.integers(0, 256, (24, 40), dtype=np.uint8)}
    maps['albedo'][3:9] = maps['albedo'][2]                         # smooth stretches: PIL then chooses row filters other than 0
    maps['albedo'][10:14, :, :] = (np.arange(40, dtype=np.uint8) * 3)[None, :, None]
    writers = [False] + ([True] if _have_pil() else [])
    for use_pil in writers:
        d = tmp_path / f'pil_{use_pil}'
        obj = TX.write_textured_obj(str(d), v, f, vt, ft, maps, name='mesh_0', use_pil=use_pil)
        assert sorted(os.listdir(d)) == ['feat0_0.png', 'feat1_0.png', 'feat2_0.png', 'mesh_0.mtl', 'mesh_0.obj']
        back = TX.read_textured_obj(obj)
        assert np.array_equal(back['vt'], vt) and np.array_equal(back['ft'], ft) and np.array_equal(back['f'], f)
        assert np.allclose(back['v'], v, rtol=1e-8, atol=0) and np.array_equal(back['v'].astype(np.float32), v.astype(np.float32))
        assert back['map_Kd'] == 'feat0_0.png' and back['mtllib'] == 'mesh_0.mtl'
        for k in maps:
            assert np.array_equal(back[k], maps[k]), (use_pil, k)
        text = open(obj).read().split('\n')
        first_face = next(ln for ln in text if ln.startswith('f '))
        assert text[0] == 'mtllib mesh_0.mtl' and text[1].startswith('v ')
        assert first_face == 'f ' + ' '.join(f'{f[0, k] + 1}/{ft[0, k] + 1}' for k in range(3))       # 1-based a/b
        u0, v0 = (float(x) for x in next(ln for ln in text if ln.startswith('vt ')).split()[1:])
        assert u0 == float(vt[0, 0]) and v0 == 1.0 - float(vt[0, 1])                # vt u 1-v
        if use_pil:                                                 # both writers decode to the same arrays, through PIL's decoder too
            from PIL import Image
            for name, key in (('feat0_0.png', 'albedo'), ('feat1_0.png', 'metallic')):
                a = np.asarray(Image.open(d / name))
                b = np.asarray(Image.open(tmp_path / 'pil_False' / name))
                assert np.array_equal(a, b) and np.array_equal(a[..., 0] if key != 'albedo' else a, maps[key])


def test_texture_symbols_are_exported():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(os.path.join(ge.ROOT, 'nero_amd', 'libnero_hip.so'))
    for n in ('nero_uv_raster_workspace_bytes', 'nero_uv_raster', 'nero_uv_interp_workspace_bytes', 'nero_uv_interp', 'nero_tex_quantize',
              'nero_tex_regions_workspace_bytes', 'nero_tex_regions', 'nero_tex_fill', 'nero_tex_downsample2'):
        assert hasattr(lib, n), n
    hdr = open(os.path.join(ge.ROOT, 'include', 'nero_hip.h')).read()
    assert 'int nero_tex_fill(' in hdr and 'int nero_uv_raster(' in hdr
