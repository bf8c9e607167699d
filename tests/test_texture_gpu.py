"""GPU tier of the texture baking: every kernel of nero_amd/csrc/texture.hip against its numpy restatement (tests/texture_ref.py) and against what
scipy / sklearn recorded (tests/golden/texture_regions.npz), then NeROMaterialRenderer.extract_texture_maps end to end."""
import os

import numpy as np
import pytest
import torch

from tests import texture_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'texture_regions.npz')
ERR_ARG = 'libnero_hip error -1'


@pytest.fixture(scope='module')
def TX():
    from nero_amd import texture
    return texture


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ---- raster -----------------------------------------------------------------------------------------------------------------------------------
def _raster_cases():
    cases = {}
    for h, w, nx, ny, seed in R.GRID_CASES:
        cases[f'grid_{h}x{w}'] = R.jittered_grid(h, w, nx, ny, seed) + (h, w)
    for name, (vt, ft, h, w, _) in R.special_cases().items():
        cases[name] = (vt, ft, h, w)
    f32 = lambda a: np.array(a, np.float32)
    cases['two_triangles_512'] = (f32([[0, 0], [1, 0], [1, 1], [0, 1]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32), 512, 512)
    rng = np.random.default_rng(7)                                 # 20 000 triangles with edges of 0.2 - 3 texels on 257 x 130: most cover nothing
    h, w, n = 257, 130, 20000
    c = rng.random((n, 1, 2)) * np.array([w, h])
    ang = rng.random((n, 1)) * 2 * np.pi + np.array([[0.0, 2.1, 4.2]]) + rng.normal(0, 0.3, (n, 3))
    rad = rng.uniform(0.2, 3.0, (n, 1)) / np.sqrt(3) * rng.uniform(0.7, 1.0, (n, 3))
    p = c + np.stack([np.cos(ang), np.sin(ang)], -1) * rad[..., None]
    cases['small_random_20000'] = ((p / np.array([w, h])).reshape(-1, 2).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3), h, w)
    # vertices outside [0, 1], by a little and by a lot; a non-finite vertex and one beyond 2^30 make their triangles cover nothing
    cases['outside_unit_square'] = (f32([[-0.5, -0.25], [1.7, 0.2], [0.3, 2.5], [-40.0, 0.5], [0.5, -30.0], [60.0, 55.0], [np.nan, 0.5], [0.2, 0.2],
                                         [0.8, 0.3], [1e9, 0.1], [np.inf, 0.4]]),
                                    np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 7, 8], [10, 8, 7]], np.int32), 40, 56)
    big = R.jittered_grid(1, 37, 5, 2, 4)
    cases['h_of_1'] = big + (1, 37)
    cases['w_of_1'] = R.jittered_grid(29, 1, 2, 5, 5) + (29, 1)
    cases['mid_size_mix'] = R.jittered_grid(200, 150, 9, 7, 6) + (200, 150)     # boxes of ~500 texels: every triangle goes through the block walk
    return cases


RASTER_CASES = _raster_cases()


@pytest.mark.parametrize('name', list(RASTER_CASES))
def test_rasterize_uv_equals_the_rule_bit_for_bit(TX, name):
    vt, ft, h, w = RASTER_CASES[name]
    ref = R.raster(vt, ft, h, w)
    got = TX.rasterize_uv(vt, ft, h, w)
    assert got.dtype == torch.int32 and tuple(got.shape) == (h, w)
    assert torch.equal(got.cpu(), torch.from_numpy(ref)), (name, int((got.cpu() != torch.from_numpy(ref)).sum()))
    if name == 'small_random_20000':
        hit = np.unique(ref[ref >= 0]).size
        assert 0 < hit < 0.6 * len(ft)                              # most triangles cover no centre
    if name == 'two_triangles_512':
        assert (ref >= 0).all()
    assert torch.equal(TX.rasterize_uv(vt, ft, h, w), got)          # atomics decide nothing: the same bits again


def test_rasterize_uv_refuses_bad_arguments_and_writes_nothing(TX):
    from nero_amd._lib import NeroHipError
    vt, ft, h, w = RASTER_CASES['grid_8x8']
    for hh, ww in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        with pytest.raises(NeroHipError, match=ERR_ARG):
            TX.rasterize_uv(vt, ft, hh, ww)
    out = torch.full((8, 8), 12345, dtype=torch.int32, device='cuda')
    for bad_value in (len(vt), -1):
        bad = ft.copy()
        bad[3, 1] = bad_value
        with pytest.raises(NeroHipError, match=ERR_ARG):
            TX.rasterize_uv(vt, bad, 8, 8, out=out)
        assert bool((out == 12345).all())
    for kw in (dict(pad=65), dict(pad=-1), dict(border=0), dict(border=17)):
        with pytest.raises(NeroHipError, match=ERR_ARG):
            TX.gutter_regions(torch.ones((8, 8), dtype=torch.uint8, device='cuda'), **kw)


# ---- interpolation ----------------------------------------------------------------------------------------------------------------------------
def test_interpolate_compacts_in_order_and_rounds_once(TX):
    from nero_amd._lib import NeroHipError
    h, w = 33, 20
    vt, ft = R.jittered_grid(h, w, 7, 5, 3)
    ft = ft[np.arange(len(ft)) % 5 != 2]                            # holes: some texels stay uncovered
    rng = np.random.default_rng(3)
    nv = 50
    attr = (rng.normal(0, 1, (nv, 4)) * np.array([1.0, 100.0, 1e-3, 7.0])).astype(np.float32)
    fa = rng.integers(0, nv, ft.shape).astype(np.int32)            # its own face array
    tri_id = TX.rasterize_uv(vt, ft, h, w)
    texel, vals, mask = TX.interpolate(tri_id, vt, ft, attr, fa, return_mask=True)
    r_texel, r_vals, _ = R.interp(tri_id.cpu().numpy(), vt, ft, attr, fa)
    assert 0 < len(r_texel) < h * w
    assert texel.dtype == torch.int32 and torch.equal(texel.cpu(), torch.nonzero(tri_id.reshape(-1) >= 0)[:, 0].int().cpu())
    assert np.array_equal(texel.cpu().numpy(), r_texel) and bool((texel[1:] > texel[:-1]).all())
    assert torch.equal(mask.cpu(), (tri_id >= 0).to(torch.uint8).cpu())
    err = np.abs(vals.cpu().numpy().astype(np.float64) - r_vals)
    bound = 2.0 ** -23 * np.abs(attr).max(axis=0)                   # one rounding to fp32: one ulp at the largest magnitude, per component
    print('interpolate: max |err| / bound per component', (err.max(axis=0) / bound).tolist(),
          'bit-equal to the rounded float64 value:', bool(np.array_equal(vals.cpu().numpy(), r_vals.astype(np.float32))))
    assert np.all(err <= bound[None, :])
    # a capacity one short: NERO_ERR_ARG, outputs untouched
    n = len(r_texel)
    t_buf = torch.full((n - 1,), -7, dtype=torch.int32, device='cuda')
    v_buf = torch.full((n - 1, 4), -7.0, dtype=torch.float32, device='cuda')
    with pytest.raises(NeroHipError, match=ERR_ARG):
        TX.interpolate(tri_id, vt, ft, attr, fa, out=(t_buf, v_buf))
    assert bool((t_buf == -7).all()) and bool((v_buf == -7.0).all())
    bad = fa.copy()
    bad[0, 0] = nv
    with pytest.raises(NeroHipError, match=ERR_ARG):
        TX.interpolate(tri_id, vt, ft, attr, bad, out=(t_buf, v_buf))
    assert bool((t_buf == -7).all()) and bool((v_buf == -7.0).all())
    t2, v2 = TX.interpolate(tri_id, vt, ft, attr, fa, cap=n + 5)    # room to spare: the same rows
    assert torch.equal(t2, texel) and torch.equal(v2, vals)


# ---- regions ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', range(len(R.GUTTER_MASKS)))
@pytest.mark.parametrize('pad', R.GUTTER_PADS)
def test_gutter_regions_equal_scipy(TX, gold, m, pad):
    got = TX.gutter_regions(cu(gold[f'mask_{m}']), pad=pad, border=3)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(gold[f'region_{m}_{pad}']))


@pytest.mark.parametrize('pad,border', [(64, 16), (0, 3), (17, 1)])
def test_gutter_regions_at_the_limits(TX, pad, border):
    rng = np.random.default_rng(21)
    h, w = 301, 517                                                 # more than one row segment, no multiple of any tile
    mask = np.zeros((h, w), bool)
    for _ in range(9):
        rh, rw = rng.integers(3, 90), rng.integers(3, 120)
        y, x = rng.integers(0, h - rh), rng.integers(0, w - rw)
        mask[y:y + rh, x:x + rw] = True
    mask[100:140, 200:260] &= rng.random((40, 60)) < 0.7            # holes
    mask |= rng.random((h, w)) < 0.0005
    mask[:, -1] |= rng.random(h) < 0.3                              # texels on the image edge
    got = TX.gutter_regions(cu(mask.astype(np.uint8)), pad=pad, border=border)
    assert torch.equal(got.cpu(), torch.from_numpy(R.regions(mask, pad, border)))


# ---- fill -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fill_refs(gold):
    """texture_ref.fill of a 5-channel map on every fixture region, computed once"""
    out = {}
    for m, (h, w, _) in enumerate(R.GUTTER_MASKS):
        rng = np.random.default_rng(100 + m)
        tex = rng.integers(1, 256, (h, w, 5), dtype=np.uint8)
        for pad in R.GUTTER_PADS:
            region = gold[f'region_{m}_{pad}']
            out[(m, pad)] = (tex, region) + R.fill(tex, region, pad)
    return out


@pytest.mark.parametrize('m', range(len(R.GUTTER_MASKS)))
@pytest.mark.parametrize('pad', R.GUTTER_PADS)
def test_fill_gutter_equals_the_reference(TX, gold, fill_refs, m, pad):
    from nero_amd.eval_shape import nearest_dist
    tex, region, r_tex, r_src = fill_refs[(m, pad)]
    h, w = region.shape
    for C in (5, 1):
        t_in = tex if C == 5 else tex[..., :1]
        t = cu(t_in.copy())
        res, src = TX.fill_gutter(t, cu(region), pad=pad, return_source=True)
        assert res.data_ptr() == t.data_ptr()                       # in place
        assert torch.equal(src.cpu(), torch.from_numpy(r_src))
        assert torch.equal(res.cpu(), torch.from_numpy(r_tex if C == 5 else r_tex[..., :1]))
        assert torch.equal(res.cpu()[torch.from_numpy(region != 3)], torch.from_numpy(t_in[region != 3]))        # nothing else was touched
    t1 = cu(tex[..., 0].copy())                                     # a 2-D map, no source requested
    assert torch.equal(TX.fill_gutter(t1, cu(region), pad=pad).cpu(), torch.from_numpy(r_tex[..., 0]))
    # cross-checks of the chosen distance: the project's brute-force nearest neighbour, and sklearn's kd-tree (fixture)
    fy, fx = np.nonzero(region == 3)
    s = src.cpu().numpy()[fy, fx].astype(np.int64)
    assert (s >= 0).all() and (region.reshape(-1)[s] == 2).all()
    d2 = (s // w - fy) ** 2 + (s % w - fx) ** 2
    assert np.array_equal(d2, gold[f'd2_{m}_{pad}'].astype(np.int64))
    sy, sx = np.nonzero(region == 2)
    z = lambda a, b: np.stack([a, b, np.zeros_like(a)], -1).astype(np.float32)
    nn = nearest_dist(cu(z(fy, fx)), cu(z(sy, sx))).cpu().numpy().astype(np.float64)
    assert np.array_equal(np.rint(nn ** 2).astype(np.int64), d2) and np.abs(nn ** 2 - d2).max() < 1e-2


def test_fill_gutter_leaves_an_inconsistent_region_alone(TX):
    h, w = 40, 50
    region = np.zeros((h, w), np.uint8)
    region[5:20, 7:30] = 3                                          # fill texels, no search texel anywhere
    region[30:, 40:] = 1
    tex = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    t = cu(tex.copy())
    _, src = TX.fill_gutter(t, cu(region), pad=64, return_source=True)
    assert torch.equal(t.cpu(), torch.from_numpy(tex)) and bool((src == -1).all())
    region[39, 49] = 2                                              # a search texel outside every window of pad 8: still nothing
    _, src = TX.fill_gutter(t, cu(region), pad=8, return_source=True)
    assert torch.equal(t.cpu(), torch.from_numpy(tex)) and bool((src == -1).all())


# ---- quantise / downsample ------------------------------------------------------------------------------------------------------------------------
def test_quantize_matches_float64_srgb(TX):
    rng = np.random.default_rng(9)
    h, w, C = 37, 45, 5
    n = 1500
    texel = np.sort(rng.choice(h * w, n, replace=False)).astype(np.int32)
    vals = rng.random((n, C)).astype(np.float32)
    vals[:40] = rng.random((40, C)).astype(np.float32) * 0.005      # around the linear / power switch
    vals[40, :] = [0.0, 1.0, 0.0031308, np.float32(0.0031308) + np.float32(1e-9), 0.5]
    vals[41, :] = [np.nan, -3.0, 7.5, np.inf, -np.inf]
    vals[42, :] = [-0.0, 1e-30, 1.0 - 2.0 ** -24, 2.0 ** -23, 0.999]
    got = TX.quantize(vals, texel, h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, C)
    g = got.cpu().numpy().reshape(h * w, C)
    s = R.srgb255(vals.astype(np.float64))
    ref = s.astype(np.uint8)
    assert np.abs(g[texel].astype(np.int32) - ref.astype(np.int32)).max() <= 1
    far = np.abs(s - np.rint(s)) > 1e-3
    assert far.mean() > 0.9 and np.array_equal(g[texel][far], ref[far])
    print('quantize: levels differing from float64 numpy:', int((g[texel] != ref).sum()), 'of', ref.size)
    assert np.array_equal(g[texel][41], [0, 0, 255, 255, 0]) and np.array_equal(g[texel][40][:2], [0, 255])
    rest = np.ones(h * w, bool)
    rest[texel] = False
    assert (g[rest] == 0).all()


@pytest.mark.parametrize('shape', [(2, 2, 3), (130, 258, 5), (6, 10)])
def test_downsample2_equals_the_reference(TX, shape):
    rng = np.random.default_rng(shape[1])
    tex = rng.integers(0, 256, shape, dtype=np.uint8)
    tex[:2, :2] = np.array([[255, 255], [255, 254]], np.uint8).reshape((2, 2) + (1,) * (len(shape) - 2))     # odd sums, the top of the range
    tex[0::2, 2:4] = 1                                             # sums of 2 and 1: the rounding
    got = TX.downsample2(cu(tex))
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(R.downsample2(tex)))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def baked():
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import build_material_case, golden_mesh, load_golden
    _, meta = load_golden('mat_bell')
    ref = build_material_case(meta)
    net = NeROMaterialRenderer({'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell'}, mesh=golden_mesh())
    net.load_state_dict(ref.state_dict())
    net = net.cuda()
    first = net.extract_texture_maps(size=128, ssaa=2, return_intermediates=True)
    n = first['points'].shape[0]
    chunk = n // 3 - 7                                              # four chunks, the last one ragged
    assert n > 1280 and chunk > 0 and n % chunk != 0 and -(-n // chunk) >= 3
    second = net.extract_texture_maps(size=128, ssaa=2, chunk=chunk, return_intermediates=True)
    return net, first, second, chunk


def test_bake_shapes_dtypes_and_determinism(baked):
    net, a, b, _ = baked
    assert tuple(a['albedo'].shape) == (128, 128, 3) and tuple(a['metallic'].shape) == (128, 128) and tuple(a['roughness'].shape) == (128, 128)
    assert all(a[k].dtype == torch.uint8 and a[k].is_cuda and a[k].is_contiguous() for k in ('albedo', 'metallic', 'roughness'))
    assert a['mask'].dtype == torch.bool and tuple(a['mask'].shape) == (128, 128) and 0 < int(a['mask'].sum()) < 128 * 128
    assert a['vt'].shape == (3 * 1280, 2) and a['ft'].shape == (1280, 3)
    for k in ('albedo', 'metallic', 'roughness', 'mask', 'tri_id', 'texel', 'points', 'values', 'region', 'source', 'texture'):
        assert torch.equal(a[k], b[k]), k                           # two runs (and two chunkings) are bit-identical
    assert np.array_equal(np.unique(a['tri_id'].cpu().numpy()), np.arange(-1, 1280))       # every triangle owns texels


def test_bake_points_lie_on_their_triangles(baked):
    net, a, _, _ = baked
    v, f = net.mesh_vertices.astype(np.float64), net.mesh_triangles
    tri = a['tri_id'].reshape(-1)[a['texel'].long()].cpu().numpy()
    p = a['points'].cpu().numpy().astype(np.float64)
    A, B, Cc = v[f[tri, 0]], v[f[tri, 1]], v[f[tri, 2]]
    # barycentric coordinates by least squares in the triangle's plane, float64
    e1, e2, d = B - A, Cc - A, p - A
    g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    r1, r2 = (d * e1).sum(-1), (d * e2).sum(-1)
    det = g11 * g22 - g12 * g12
    b1, b2 = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    b0 = 1.0 - b1 - b2
    recon = b0[:, None] * A + b1[:, None] * B + b2[:, None] * Cc
    assert min(b0.min(), b1.min(), b2.min()) >= -1e-6
    assert np.abs(recon - p).max() <= 1e-6                          # on the plane
    # three free weights, p = w0 A + w1 B + w2 C (the vertices are independent vectors: the mesh surrounds the origin): their sum is 1
    wgt = np.linalg.solve(np.stack([A, B, Cc], -1), p[..., None])[..., 0]
    print(f'bake: barycentric weights min {wgt.min():.3e}, |sum - 1| max {np.abs(wgt.sum(-1) - 1).max():.3e}')
    assert wgt.min() >= -1e-6 and np.abs(wgt.sum(-1) - 1).max() <= 1e-6
    _, r_vals, r_bary = R.interp(a['tri_id'].cpu().numpy(), a['vt'], a['ft'], net.mesh_vertices, net.mesh_triangles)
    assert np.abs(r_bary.sum(-1) - 1).max() <= 1e-12 and r_bary.min() >= 0
    assert np.array_equal(a['points'].cpu().numpy(), r_vals.astype(np.float32))
    assert np.abs(np.stack([b0, b1, b2], -1) - r_bary).max() <= 1e-5


def test_bake_values_equal_one_direct_call(baked):
    net, a, b, chunk = baked
    with torch.no_grad():
        m, r, alb = net.predict_materials(a['points'].contiguous())
    direct = torch.cat([alb, m, r], 1)
    err = float((b['values'] - direct).abs().max())
    print(f'bake: chunked ({chunk} rows per chunk) vs one direct predict_materials call: max |diff| {err:.3e}, bit-equal {torch.equal(b["values"], direct)}')
    assert err <= 1e-6
    assert float(direct[:, 4].min()) >= 0.04 ** 2 - 1e-7             # the network's roughness, no square root applied


def test_bake_pipeline_equals_the_reference_on_the_same_values(baked):
    net, a, _, _ = baked
    H = W = 256
    vals = a['values'].cpu().numpy()
    texel = a['texel'].cpu().numpy()
    tri_id = a['tri_id'].cpu().numpy()
    assert np.array_equal(tri_id, R.raster(a['vt'], a['ft'], H, W))
    tex = R.quantize(vals, texel, H, W)
    region = R.regions(tri_id >= 0, 32, 3)
    assert np.array_equal(a['region'].cpu().numpy(), region)
    filled, src = R.fill(tex, region, 32)
    assert np.array_equal(a['source'].cpu().numpy(), src)
    assert np.array_equal(a['texture'].cpu().numpy(), filled)
    small = R.downsample2(filled)
    assert np.array_equal(a['albedo'].cpu().numpy(), small[..., :3])
    assert np.array_equal(a['metallic'].cpu().numpy(), small[..., 3]) and np.array_equal(a['roughness'].cpu().numpy(), small[..., 4])
    # every texel within city-block distance 32 of a chart is filled from a chart texel: non-zero wherever its source is
    near = (R.cityblock_to(tri_id >= 0) <= 32) & (tri_id < 0)
    s = a['source'].cpu().numpy()
    assert near.sum() > 1000 and (s[near] >= 0).all() and (s[~near] == -1).all()
    t = a['texture'].cpu().numpy().reshape(H * W, 5)
    assert np.array_equal(t[near.reshape(-1)], t[s[near]])
    assert np.all((t[near.reshape(-1)] != 0) == (t[s[near]] != 0)) and (t[s[near]] != 0).any()


def test_bake_with_an_explicit_atlas_equals_the_default(baked, TX):
    net, a, _, _ = baked
    vt, ft = TX.simple_atlas(net.mesh_vertices, net.mesh_triangles, 128)
    c = net.extract_texture_maps(vt=torch.from_numpy(vt).cuda(), ft=ft, size=128, ssaa=2)
    for k in ('albedo', 'metallic', 'roughness', 'mask'):
        assert torch.equal(a[k], c[k]), k
    d = net.extract_texture_maps(size=128, ssaa=1, pad=5)
    assert tuple(d['albedo'].shape) == (128, 128, 3) and int(d['mask'].sum()) > 1280 - 1
    with pytest.raises(ValueError):
        net.extract_texture_maps(size=128, ssaa=3)
