"""GPU tier of the texture lookup (include/nero_hip_texfetch.h, nero_amd/csrc/tex_fetch.hip, nero_amd/texfetch.py, Relighter(textures=...)):
the pyramid against repeated texture.downsample2, the face scale, the fetch's decisions bit for bit against the float32 restatement
(tests/texfetch_ref.py) and its values against the float64 one, constant maps, the per-vertex stand-in, and the relighter end to end.

NO LANE READS OUT OF RANGE: every fetch here reads a pyramid that ends where its allocation ends (_texture_set), with coordinates at 0 and
1, outside [0, 1] and not finite among the inputs.  The argument is the kernel's index arithmetic, not the absence of a fault: a record is
addressed as off[k] + y w_k + x with y clamped to [0, h_k - 1] and x to [0, w_k - 1] (clamp_index in tex_fetch.hip, after the coordinate
itself was clamped to [-1, n] as a float, so the conversion to an integer cannot overflow), off[k] + h_k w_k <= records
(tests/tex_fetch_plan_main.cpp), and the level k is min(exponent, L - 1) >= 0, with k + 1 read only where k < L - 1."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import relight_ref as RR
from tests import texfetch_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END_BUFFER = 20 << 20          # bytes: large enough that the caching allocator asks the device for a block of its own


@pytest.fixture(scope='module')
def TF():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import texfetch
    return texfetch


@pytest.fixture(scope='module')
def RL(TF):
    from nero_amd import relight
    return relight


def _texture_set(TF, maps):
    """the maps' TextureSet with its pyramid in the last bytes of a buffer"""
    h, w = maps[1].shape
    need = 8 * sum((h >> k) * (w >> k) for k in range(TR.levels(h, w)))
    buf = torch.empty(END_BUFFER, dtype=torch.uint8, device='cuda')
    tex = TF.TextureSet(*maps, out=buf[END_BUFFER - need:])
    tex._buffer = buf
    assert tex.pyramid.data_ptr() + need == buf.data_ptr() + END_BUFFER and tex.pyramid.data_ptr() % 8 == 0
    return tex


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. pyramid -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', TR.SIZES)
def test_every_level_is_repeated_downsample2(TF, h, w):
    from nero_amd.texture import downsample2
    maps = TR.random_maps(h, w)
    tex = _texture_set(TF, maps)
    want = TR.pyramid(*maps)
    assert tex.levels == len(want) == TR.levels(h, w) and tex.pyramid.numel() == 8 * sum(l.shape[0] * l.shape[1] for l in want)
    below = torch.from_numpy(np.ascontiguousarray(want[0][..., :5])).cuda()
    for k in range(tex.levels):
        got = tex.level(k)
        assert tuple(got.shape) == (h >> k, w >> k, 8)
        if k > 0:
            below = downsample2(below)
        assert torch.equal(got[..., :5], below), k                                   # the device's own downsample2, applied k times
        assert not bool(got[..., 5:].any())                                          # the padding bytes stay 0
        assert np.array_equal(got.cpu().numpy(), want[k])
    with pytest.raises(IndexError):
        tex.level(tex.levels)


# ---- 2. face scale --------------------------------------------------------------------------------------------------------------------------
def test_face_scale(TF):
    quad_v = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    quad_f = np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
    quad_vt = np.asarray([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    for size in (1, 8, 64, 1000, 16384):                                              # a unit quad mapped to the whole map: w exactly
        assert TF.face_scale(quad_v, quad_f, quad_vt, quad_f, size, size).tolist() == [float(size)] * 2
    assert TF.face_scale(3.0 * quad_v, quad_f, quad_vt, quad_f, 96, 96).tolist() == [32.0, 32.0]
    got = TF.face_scale(quad_v, quad_f, quad_vt, quad_f, 96, 80).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(TR.face_scale(quad_v, quad_f, quad_vt, quad_f, 96, 80))) and abs(got[0] - np.sqrt(96 * 80)) < 1e-5
    # degenerate and out-of-range faces give 0 (the vertex arrays end where the allocation's contents end: nothing is read through them)
    tris = np.asarray([[0, 1, 2], [0, 0, 2], [0, 1, 2], [0, 1, 4], [-1, 1, 2], [0, 1, 2], [0, 1, 2], [0, 2, 3]], np.int32)
    ft = np.asarray([[0, 1, 2], [0, 1, 2], [1, 1, 2], [0, 1, 2], [0, 1, 2], [0, 4, 2], [0, 1, -7], [0, 2, 3]], np.int32)
    assert TF.face_scale(quad_v, tris, quad_vt, ft, 64, 64).tolist() == [64.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 64.0]
    bad_v = quad_v.copy()
    bad_v[3] = (np.nan, 0, 0)
    huge = 1e30 * quad_v
    assert TF.face_scale(bad_v, quad_f, quad_vt, quad_f, 64, 64).tolist() == [64.0, 0.0]
    assert TF.face_scale(huge, quad_f, quad_vt, quad_f, 64, 64).tolist() == [0.0, 0.0]                 # the world area overflows: 0, not NaN
    assert TF.face_scale(quad_v, quad_f[:0], quad_vt, quad_f[:0], 64, 64).numel() == 0
    # a mesh: the float32 restatement bit for bit
    V, F = RR.scene(subdiv=2)
    from nero_amd.texture import simple_atlas
    vt, ft = simple_atlas(V.numpy(), F.numpy(), 64)
    got = TF.face_scale(V, F, vt, ft, 64, 64).cpu().numpy()
    want = TR.face_scale(V.numpy(), F.numpy(), vt, ft, 64, 64)
    assert np.array_equal(_bits(got), _bits(want)) and (got > 0).all()


# ---- 3. the fetch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', TR.SIZES)
def test_the_fetch_decides_as_the_restatement_and_stays_within_the_measured_floor(TF, h, w):
    maps = TR.random_maps(h, w)
    tex = _texture_set(TF, maps)
    lv, lut = TR.pyramid(*maps), TR.srgb_lut()
    tol = TR.GPU_FACTOR * TR.F32_FLOOR
    worst = 0.0
    for n in TR.NS:
        c = TR.fetch_case(h, w, n)
        for spread, bias in TR.LODS:
            mat5, dbg = TF.fetch_materials(tex, c['vt'], c['ft'], c['scale'], c['face'], c['bary'], c['depth'], spread, bias, return_debug=True)
            assert tuple(mat5.shape) == (n, 5) and tuple(dbg.shape) == (n, 8)
            if n == 0:
                continue
            mat5, dbg = mat5.cpu().numpy(), dbg.cpu().numpy()
            m32, d32 = TR.fetch(lv, lut, spread=spread, lod_scale=2.0 ** bias, dtype=np.float32, **c)
            m64, _ = TR.fetch(lv, lut, spread=spread, lod_scale=2.0 ** bias, dtype=np.float64, **c)
            assert np.array_equal(_bits(dbg[:, :6]), _bits(d32[:, :6])), (n, spread, bias)           # l, t, x0, y0, fx, fy: bit for bit
            assert np.array_equal(dbg[:, 6:], d32[:, 6:], equal_nan=True)                            # uv (a NaN's payload is not compared)
            assert np.isfinite(mat5).all()
            err = float(np.abs(mat5.astype(np.float64) - m64).max())
            worst = max(worst, err)
            assert err <= tol, (n, spread, bias, err, tol)
            assert np.array_equal(_bits(mat5), _bits(m32)), (n, spread, bias)                        # nothing is ordered differently
            k = len(TR.SPECIAL_UV)
            if n >= k + 4:
                assert not mat5[k:k + 4].any() and not dbg[k:k + 4].any()                            # face -1, face T, two bad UV indices
    print(f'{h} x {w}: max |GPU - float64| {worst:.3e} (floor {TR.F32_FLOOR:.3e}, bound {tol:.3e})')
    # the plain call, and spread=None: level 0
    c = TR.fetch_case(h, w, 65)
    a = TF.fetch_materials(tex, c['vt'], c['ft'], c['scale'], c['face'], c['bary'], c['depth'])
    b, d = TF.fetch_materials(tex, c['vt'], c['ft'], c['scale'], c['face'], c['bary'], c['depth'], 0.0, return_debug=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not bool(d[:, :2].any())


def test_constant_maps_return_their_decoded_value_at_every_level_of_detail(TF):
    lut = TR.srgb_lut()
    g = np.random.default_rng(11)
    n = 1000
    vt = np.asarray([[0, 0], [1, 0], [0, 1], [1, 1], [-0.5, 2.0]], np.float32)
    ft = np.asarray([[0, 1, 2], [3, 2, 1], [4, 0, 3]], np.int32)
    bary = g.uniform(0, 1, (n, 2)).astype(np.float32)
    bary[:, 1] *= 1 - bary[:, 0]
    depth = np.exp2(g.uniform(-3, 12, n)).astype(np.float32)
    face = g.integers(0, 3, n).astype(np.int32)
    scale = np.asarray([1.0, 3.0, 0.7], np.float32)
    for (h, w), byte in (((1, 1), (0, 0, 0, 0, 0)), ((6, 10), (13, 128, 255, 200, 77)), ((64, 64), (255, 1, 10, 11, 254)), ((96, 80), (40, 41, 42, 43, 44))):
        alb = np.empty((h, w, 3), np.uint8)
        alb[:] = byte[:3]
        tex = _texture_set(TF, (alb, np.full((h, w), byte[3], np.uint8), np.full((h, w), byte[4], np.uint8)))
        want = np.asarray([lut[byte[3]], np.sqrt(lut[byte[4]]), lut[byte[0]], lut[byte[1]], lut[byte[2]]], np.float32)
        seen = set()
        for spread, bias in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (1e30, 0.0)):
            mat5, dbg = TF.fetch_materials(tex, vt, ft, scale, face, bary, depth, spread, bias, return_debug=True)
            assert np.array_equal(_bits(mat5.cpu().numpy()), _bits(np.broadcast_to(want, (n, 5)))), ((h, w), spread, bias)
            seen |= set(dbg[:, 0].cpu().numpy().astype(int).tolist())
        assert seen == set(range(tex.levels))                                       # every level was visited


# ---- 4. the per-vertex stand-in -------------------------------------------------------------------------------------------------------------
def test_vertex_materials(TF):
    from nero_amd.texture import simple_atlas
    V, F = RR.scene(subdiv=2)
    V, F = V.numpy(), F.numpy()
    nV = len(V) + 3                                                                  # three vertices no face names
    vt, ft = simple_atlas(V, F, 64)
    maps = TR.random_maps(64, 64, seed=1)
    tex = _texture_set(TF, maps)
    want, owner_want = TR.vertex_materials(TR.pyramid(*maps), TR.srgb_lut(), vt, F, ft, nV)
    got, owner = TF.vertex_materials(tex, vt, F, ft, nV, return_owner=True)
    assert np.array_equal(owner.cpu().numpy(), owner_want) and (owner_want[-3:] == TR.NO_OWNER).all() and (owner_want[:-3] < 3 * len(F)).all()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and not got[-3:].any() and bool(got[:-3].any(1).all())
    for _ in range(3):                                                               # the same on every run
        assert torch.equal(TF.vertex_materials(tex, vt, F, ft, nV).view(torch.int32), got.view(torch.int32))
    # a permutation of the faces that keeps every vertex's lowest corner: the faces that own a vertex first, in their order, the others
    # behind them in reverse
    owners = np.unique(owner_want[:-3] // 3)
    others = np.setdiff1d(np.arange(len(F)), owners)[::-1]
    assert len(others) > 50
    perm = np.concatenate([owners, others])
    again, owner2 = TF.vertex_materials(tex, vt, F[perm], ft[perm], nV, return_owner=True)
    assert not np.array_equal(owner2.cpu().numpy(), owner_want)                      # the corner numbers moved ...
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))               # ... the materials did not
    # a bad UV index at an owning corner gives zeros, an index of tris out of range is passed over
    ft_bad, F_bad = ft.copy(), F.copy()
    ft_bad[0, 0] = len(vt)
    F_bad[1, 2] = nV
    got_bad = TF.vertex_materials(tex, vt, F_bad, ft_bad, nV).cpu().numpy()
    want_bad = TR.vertex_materials(TR.pyramid(*maps), TR.srgb_lut(), vt, F_bad, ft_bad, nV)[0]
    assert np.array_equal(_bits(got_bad), _bits(want_bad)) and not got_bad[F[0, 0]].any()
    assert TF.vertex_materials(tex, vt, F[:0], ft[:0], 5).tolist() == [[0.0] * 5] * 5 and TF.vertex_materials(tex, vt, F, ft, 0).numel() == 0


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------
POSE = RR.relighting_poses(4, 30.0, 60.0, 2.4)[1].numpy()
KMAT = np.asarray([[40.0, 0, 16], [0, 40.0, 16], [0, 0, 1]], np.float32)
SIDE, SAMPLES = 32, (8, 8)
LOD_BIAS = 2.0                 # a chart of the atlas is one or two texels wide, under a pixel: two levels up, the view spans levels 0 and 1


@pytest.fixture(scope='module')
def asset():
    """a few hundred triangles (the scene of test_relight_gpu.py, one subdivision coarser), a simple_atlas and random 64 x 64 maps"""
    from nero_amd.texture import simple_atlas
    V, F = RR.scene(subdiv=2)
    vt, ft = simple_atlas(V.numpy(), F.numpy(), 64)
    alb, met, rgh = TR.random_maps(64, 64, seed=2)
    env = RR.proper_map(16, 32, seed=2, hot=(3, 20, 100.0))
    return dict(V=V, F=F, env=env, textures={'albedo': alb, 'metallic': met, 'roughness': rgh, 'vt': vt, 'ft': ft})


@pytest.fixture(scope='module')
def textured(RL, asset):
    rl = RL.Relighter(asset['V'], asset['F'], None, asset['env'], textures=asset['textures'], lod_bias=LOD_BIAS)
    return rl, rl.render(POSE, KMAT, SIDE, SIDE, samples=SAMPLES)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_the_textured_relighter_is_the_fetch_composed_with_relight_points(RL, TF, asset, textured):
    rl, out = textured
    assert 300 < len(asset['F']) < 400 and int(out['alpha'].sum()) > 100
    ro, rd = rl.camera_rays(POSE, KMAT, SIDE, SIDE)
    depth, face, bary = RL.trace_faces(rl.tracer, ro, rd)
    idx = torch.nonzero(face >= 0)[:, 0]
    mat5, dbg = TF.fetch_materials(rl.textures, rl.vt, rl.ft, rl.face_scale, face[idx], bary[idx], depth[idx], 1.0 / 40.0, LOD_BIAS, return_debug=True)
    assert len(set(dbg[:, 0].tolist())) > 1                                           # more than one level of detail is in the view
    sf = rl.surface(ro, rd, spread=1.0 / 40.0)
    assert torch.equal(sf['idx'], idx) and torch.equal(sf['mat5'].view(torch.int32), mat5.view(torch.int32))
    level0 = rl.surface(ro, rd)['mat5']
    assert torch.equal(level0, TF.fetch_materials(rl.textures, rl.vt, rl.ft, rl.face_scale, face[idx], bary[idx], depth[idx])) and not torch.equal(level0, mat5)
    pt = RL.point_records(sf['pts'], -rd[idx], sf['normal'], RL.estimator_materials(mat5), *RL.pixel_rotations(idx, 0))
    tab = RL.sample_table(8, 'cuda')
    rgb = RL.relight_points(rl.tracer, pt, tab, tab, rl.env, rl.convention, rl.rot, None, rl.geometry_type)[0]
    flat = lambda k: out[k].reshape(SIDE * SIDE, -1)[idx]
    assert torch.equal(flat('rgb_lin').view(torch.int32), rgb.view(torch.int32)) and float(rgb.max()) > 0
    assert torch.equal(flat('metallic'), mat5[:, 0:1]) and torch.equal(flat('roughness'), mat5[:, 1:2]) and torch.equal(flat('albedo'), mat5[:, 2:5])
    _same(out, rl.render(POSE, KMAT, SIDE, SIDE, samples=SAMPLES))                    # two renders: the same bits
    # the level of detail is the relighter's: a bias of one level changes the picture, and is the fetch with that bias
    biased = RL.Relighter(asset['V'], asset['F'], None, asset['env'], textures=asset['textures'], tracer=rl.tracer, lod_bias=LOD_BIAS + 1.0)
    want = TF.fetch_materials(rl.textures, rl.vt, rl.ft, rl.face_scale, face[idx], bary[idx], depth[idx], 1.0 / 40.0, LOD_BIAS + 1.0)
    assert torch.equal(biased.surface(ro, rd, spread=1.0 / 40.0)['mat5'], want) and not torch.equal(want, mat5)
    # the per-vertex stand-in of the bounce kernels
    assert torch.equal(rl.mat5, TF.vertex_materials(rl.textures, rl.vt, asset['F'], rl.ft, len(asset['V'])))


def test_bounces_denoising_and_supersampling_run_on_top(textured):
    rl, out = textured
    for kw in (dict(bounces=1), dict(denoise=True), dict(bounces=1, denoise=True, samples=(8, 8, 8)), dict(ssaa=2)):
        pic = rl.render(POSE, KMAT, SIDE, SIDE, **{'samples': SAMPLES, **kw})
        assert all(bool(torch.isfinite(v.float()).all()) for v in pic.values()), kw
        assert tuple(pic['rgb_lin'].shape) == (SIDE, SIDE, 3) and float(pic['rgb_lin'].max()) > 0
        assert torch.equal(pic['alpha'] > 0, out['alpha'] > 0) or 'ssaa' in kw
        if kw.get('bounces'):
            assert 'indirect_lin' in pic


def test_a_relighter_without_textures_takes_the_former_path(RL, asset):
    """Relighter built as before: surface() and render() against the former arithmetic written out here -- the per-vertex materials
    interpolated at the hits in torch, then point_records and relight_points"""
    V, F = asset['V'], asset['F']
    g = np.random.default_rng(0)
    mats = {'metallic': g.uniform(0, 1, (len(V), 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (len(V), 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (len(V), 3)).astype(np.float32)}
    rl = RL.Relighter(V, F, mats, asset['env'])
    assert rl.textures is None
    ro, rd = rl.camera_rays(POSE, KMAT, SIDE, SIDE)
    depth, face, bary = RL.trace_faces(rl.tracer, ro, rd)
    idx = torch.nonzero(face >= 0)[:, 0]
    f = rl.tris[face[idx].long()]
    u, v = bary[idx, 0:1], bary[idx, 1:2]
    wts = torch.stack([1.0 - u - v, u, v], 1)
    corner = rl.verts[f]
    pts = (wts * corner).sum(1)
    mat5 = (wts * torch.cat([torch.from_numpy(mats[k]) for k in ('metallic', 'roughness', 'albedo')], -1).cuda()[f]).sum(1)
    nrm = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
    nrm = torch.nn.functional.normalize(torch.where((nrm * rd[idx]).sum(-1, keepdim=True) > 0, -nrm, nrm), dim=-1)
    for sf in (rl.surface(ro, rd), rl.surface(ro, rd, spread=0.5)):                   # (spread is not read without textures)
        assert torch.equal(sf['idx'], idx) and torch.equal(sf['pts'], pts) and torch.equal(sf['mat5'], mat5) and torch.equal(sf['normal'], nrm)
    pt = RL.point_records(pts, -rd[idx], nrm, RL.estimator_materials(mat5), *RL.pixel_rotations(idx, 0))
    tab = RL.sample_table(8, 'cuda')
    rgb = RL.relight_points(rl.tracer, pt, tab, tab, rl.env, rl.convention, rl.rot, None, rl.geometry_type)[0]
    out = rl.render(POSE, KMAT, SIDE, SIDE, samples=SAMPLES)
    assert torch.equal(out['rgb_lin'].reshape(-1, 3)[idx].view(torch.int32), rgb.view(torch.int32))
    assert torch.equal(out['albedo'].reshape(-1, 3)[idx], mat5[:, 2:5]) and torch.equal(out['roughness'].reshape(-1, 1)[idx], mat5[:, 1:2])
    _same(out, RL.Relighter(V, F, mats, asset['env'], textures=None, lod_bias=0.0).render(POSE, KMAT, SIDE, SIDE, samples=SAMPLES))


def test_the_asset_round_trip_renders_the_same_bits(RL, asset, textured, tmp_path):
    from nero_amd.texture import read_textured_obj, write_textured_obj
    rl, out = textured
    tx = asset['textures']
    obj = write_textured_obj(str(tmp_path), asset['V'].numpy(), asset['F'].numpy(), tx['vt'], tx['ft'], tx, name='mesh_0')
    back = read_textured_obj(obj)
    assert np.array_equal(back['vt'], tx['vt']) and np.array_equal(back['albedo'], tx['albedo']) and np.array_equal(back['roughness'], tx['roughness'])
    again = RL.Relighter.from_asset(obj, asset['env'], lod_bias=LOD_BIAS)
    assert torch.equal(again.verts, rl.verts) and torch.equal(again.textures.pyramid, rl.textures.pyramid) and torch.equal(again.mat5, rl.mat5)
    _same(out, again.render(POSE, KMAT, SIDE, SIDE, samples=SAMPLES))
    os.remove(os.path.join(str(tmp_path), 'feat2_0.png'))
    with pytest.raises(ValueError, match='roughness'):
        RL.Relighter.from_asset(obj, asset['env'])


def test_the_script_relights_the_textured_asset(RL, asset, tmp_path):
    from nero_amd.envlight import write_hdr
    from nero_amd.texture import read_png, write_textured_obj
    tx = asset['textures']
    obj = write_textured_obj(str(tmp_path / 'asset'), asset['V'].numpy(), asset['F'].numpy(), tx['vt'], tx['ft'], tx, name='mesh_0')
    write_hdr(str(tmp_path / 'e.hdr'), RR.proper_map(8, 16, seed=6).numpy())
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'relight.py'), '--mesh', obj, '--textured', '--lod-bias', '0.5', '--hdr', str(tmp_path / 'e.hdr'),
           '--name', 'orbit', '--out', str(tmp_path / 'out'), '--num', '2', '--width', '32', '--height', '32', '--samples', '8', '8', '--cam_dist', '2.0']
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / 'out' / 'orbit')) == ['0.png', '1.png']
    rl = RL.Relighter.from_asset(obj, str(tmp_path / 'e.hdr'), lod_bias=0.5)
    poses = RL.poses_in_mesh_frame(RL.relighting_poses(2, 0.0, 30.0, 2.0))
    for k in range(2):
        img = read_png(str(tmp_path / 'out' / 'orbit' / f'{k}.png'))
        want = rl.render(poses[k], RL.default_K(32, 32), 32, 32, samples=(8, 8))['rgba8'].cpu().numpy()
        assert img.shape == (32, 32, 4) and 50 < int((img[..., 3] > 0).sum()) < 1000 and np.array_equal(img, want)
    bad = subprocess.run(cmd[:2] + ['--mesh', obj, '--lod-bias', '1', '--hdr', 'x', '--name', 'n'], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--lod-bias needs --textured' in bad.stderr
