"""GPU tier of detail transfer (include/nero_transfer.h, nero_amd/csrc/detail_transfer.hip, nero_amd/transfer.py, Relighter(normal_map=...)):
the kernels against the numpy restatement (tests/transfer_ref.py) bit for bit, the bake on an identity and on a bumpy source, the round
trip through the lookup, and the relighter with the map.

The meshes: synthetic.icosphere(2) is the target (320 faces, radius 0.5), synthetic.icosphere(4, bumps=0.03) the source (5120 faces)."""
import os

import numpy as np
import pytest
import torch

from tests import relight_ref as RR
from tests import transfer_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def TF():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import transfer
    return transfer


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _mesh(subdiv, bumps=0.0):
    from nero_amd.synthetic import icosphere
    v, f = icosphere(subdiv, 0.5, bumps)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


@pytest.fixture(scope='module')
def target():
    return _mesh(2)


@pytest.fixture(scope='module')
def source():
    from nero_amd.mesh import vertex_normals
    from nero_amd.raytracing import RayTracer
    v, f = _mesh(4, 0.03)
    r = np.linalg.norm(v, axis=1)
    assert len(f) == 5120 and 0.45 < r.min() < 0.46 and 0.56 < r.max() < 0.57
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    return dict(v=v, f=f, tracer=RayTracer(vd, fd, build='device'), normals=vertex_normals(vd, fd, weight='angle', orient='outward').cpu().numpy())


@pytest.fixture(scope='module')
def detail(TF, target, source):
    """the bake of test 4, shared with the lookup and the round trip: 256 x 256, ssaa 2, both spaces"""
    return {space: TF.bake_normal_map(*target, source['tracer'], size=256, ssaa=2, space=space, return_intermediates=True)
            for space in ('tangent', 'object')}


# ---- 1. attributes_at -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3, 4, 8])
def test_attributes_at_equals_the_restatement(TF, C):
    v, f = _mesh(1)
    g = np.random.default_rng(100 + C)
    attr = g.normal(size=(len(v), C)).astype(np.float32)
    n = 1000
    face = g.integers(-2, len(f) + 2, n).astype(np.int32)
    bary = g.uniform(0, 1, (n, 2)).astype(np.float32)
    bary[:, 1] *= 1 - bary[:, 0]
    bary[:3] = [[0, 0], [1, 0], [0, 1]]
    face[:3] = 5
    f_bad = f.copy()
    f_bad[7, 1] = len(v)                                                              # a face that names a vertex out of range
    face[3] = 7
    assert (face < 0).any() and (face >= len(f)).any()
    got = TF.attributes_at(attr, f_bad, face, bary, fill=-3.5)
    assert isinstance(got, np.ndarray) and got.shape == (n, C)                        # numpy in, numpy out
    want = R.attr_at(attr, f_bad, face, bary, fill=-3.5)
    assert np.array_equal(_bits(got), _bits(want)) and (got[3] == -3.5).all() and (got[face < 0] == -3.5).all()
    dev = TF.attributes_at(torch.from_numpy(attr).cuda(), f_bad, face, bary, fill=-3.5)
    assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(_bits(dev), _bits(want))
    assert TF.attributes_at(attr, f, face[:0], bary[:0]).shape == (0, C)
    if C == 1:
        assert np.array_equal(_bits(TF.attributes_at(attr[:, 0], f_bad, face, bary, fill=-3.5)), _bits(want[:, 0]))


def test_attributes_at_closest_points_reproduce_the_points(TF):
    """nero_bvh_closest reports point = v0 + (b1 e1 + b2 e2) with ITS e1, e2; attributes_at of the vertices evaluates the same form from
    the caller's vertices.  Were the orders different at every step, each evaluation still is 2 differences (|e| <= 2 M, half an ulp:
    2 M u each, u = 2^-24), 2 products (2 M u each), their sum (|.| <= 4 M: 4 M u) and the last sum (|.| <= 5 M: 5 M u): 17 M u, so two
    evaluations are within 34 M u of each other, M the largest |coordinate|."""
    from nero_amd.raytracing import RayTracer
    v, f = _mesh(1)
    tr = RayTracer(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), build='device')
    g = np.random.default_rng(7)
    pts = g.normal(size=(1000, 3))
    pts = (pts / np.linalg.norm(pts, axis=1, keepdims=True) * g.uniform(0.3, 0.8, (1000, 1))).astype(np.float32)
    dist, face, bary, point = tr.closest(torch.from_numpy(pts).cuda())
    got = TF.attributes_at(torch.from_numpy(v).cuda(), f, face, bary)
    M = float(np.abs(v).max())
    gap = float((got - point).abs().max())
    print(f'attributes_at(verts) against closest point: {gap:.3e} (bound {34 * M * 2.0 ** -24:.3e})')
    assert bool((face >= 0).all()) and gap <= 34 * M * 2.0 ** -24


# ---- 2. uv_tangents ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('atlas', ['triangles', 'charts'])
def test_uv_tangents_equal_the_restatement(TF, target, atlas):
    from nero_amd import texture as TX
    v, f = target
    if atlas == 'charts':
        vt, ft, _ = TX.chart_atlas(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), 128)
        vt, ft = vt.cpu().numpy(), ft.cpu().numpy()
    else:
        vt, ft = TX.simple_atlas(v, f, 128)
    tangent, sign, info = TF.uv_tangents(v, f, vt, ft, return_info=True)
    want_t, want_s, want_i = R.uv_tangents(v, f, vt, ft)
    assert tangent.is_cuda and sign.dtype == torch.int8 and info.dtype == torch.int64
    assert np.array_equal(_bits(tangent), _bits(want_t)) and np.array_equal(_np(sign), want_s) and np.array_equal(_np(info), want_i)
    assert want_i[:3].tolist() == [0, 0, 0] and (np.abs(want_s) == 1).all()
    again = TF.uv_tangents(v, f, vt, ft)
    assert torch.equal(again[0].view(torch.int32), tangent.view(torch.int32)) and torch.equal(again[1], sign)
    perm = np.random.default_rng(2).permutation(len(f))
    t2, s2, i2 = TF.uv_tangents(v, f[perm], vt, ft[perm], return_info=True)
    assert torch.equal(t2.view(torch.int32), tangent.view(torch.int32)) and np.array_equal(_np(s2), want_s[perm]) and torch.equal(i2, info)
    # the tangent runs along increasing u: stepping along it in space raises u (the UV Jacobian of every face, in float64)
    P, U = v.astype(np.float64), vt.astype(np.float64)
    e1, e2 = P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]]
    du1, du2 = U[ft[:, 1], 0] - U[ft[:, 0], 0], U[ft[:, 2], 0] - U[ft[:, 0], 0]
    tc = want_t[ft[:, 0]].astype(np.float64)
    # solve tc ~ a e1 + b e2 in the face's plane, du = a du1 + b du2
    G = np.stack([np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], 1), np.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], 1)], 1)
    ab = np.linalg.solve(G, np.stack([(tc * e1).sum(1), (tc * e2).sum(1)], 1)[..., None])[..., 0]
    assert ((ab[:, 0] * du1 + ab[:, 1] * du2) > 0).all()


def test_uv_tangents_on_the_unit_square_and_on_bad_faces(TF, target):
    from nero_amd import texture as TX
    for mirror in (False, True):
        verts, tris, vt, ft = R.unit_square(mirror)
        tangent, sign, info = TF.uv_tangents(verts, tris, vt, ft, return_info=True)
        sx = -1.0 if mirror else 1.0
        assert _np(tangent).tolist() == [[sx, 0.0, 0.0]] * 4 and _np(sign).tolist() == ([-1, -1] if mirror else [1, 1]) and _np(info).tolist() == [0, 0, 0, 1]
        # B = +y in both: a map that is green above 128 tilts the normal towards +y
        nm = TF.NormalMap(np.full((4, 4, 3), (128, 204, 230), np.uint8))
        out = TF.apply_normal_map(nm, vt, ft, np.ones(2, np.float32), tangent, sign, np.asarray([0, 1], np.int32), np.full((2, 2), 0.25, np.float32),
                                  np.ones(2, np.float32), np.asarray([[0, 0, 1], [0, 0, 1]], np.float32))
        assert bool((out[:, 1] > 0.5).all()) and bool((out[:, 0].abs() < 1e-6).all()) and bool((out[:, 2] > 0.7).all())
    v, f = target
    vt, ft = TX.simple_atlas(v, f, 128)
    base_t, base_s = TF.uv_tangents(v, f, vt, ft)
    ft_bad, f_bad = ft.copy(), f.copy()
    ft_bad[0, 1] = ft_bad[0, 0]                                                       # a repeated UV index
    ft_bad[1, 2] = len(vt)                                                            # a UV index out of range
    f_bad[2, 0] = -1                                                                  # a vertex index out of range
    t3, s3, i3 = TF.uv_tangents(v, f_bad, vt, ft_bad, return_info=True)
    w3 = R.uv_tangents(v, f_bad, vt, ft_bad)
    assert np.array_equal(_bits(t3), _bits(w3[0])) and np.array_equal(_np(s3), w3[1]) and np.array_equal(_np(i3), w3[2])
    assert _np(i3)[:2].tolist() == [2, 1] and _np(s3)[:3].tolist() == [0, 0, 0] and torch.equal(s3[3:], base_s[3:])
    rest = np.setdiff1d(np.arange(len(vt)), np.concatenate([ft[0], ft[1], ft[2]]))
    assert torch.equal(t3[rest].view(torch.int32), base_t[rest].view(torch.int32))


# ---- 3. the bake, identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('atlas', ['triangles', 'charts'])
@pytest.mark.parametrize('ssaa', [1, 2])
def test_baking_a_mesh_onto_itself_gives_a_flat_map(TF, target, atlas, ssaa):
    v, f = target
    size, pad = 128, 32
    out = TF.bake_normal_map(v, f, (v, f), size=size, ssaa=ssaa, pad=pad, atlas=atlas, return_intermediates=True)
    assert out['unmatched'] == 0 and out['max_moved'] < 1e-6 and out['space'] == 'tangent' and out['normals'] == 'angle'
    assert tuple(out['normal'].shape) == (size, size, 3) and out['normal'].dtype == torch.uint8 and ('atlas_info' in out) == (atlas == 'charts')
    flat = torch.tensor(R.FLAT, dtype=torch.uint8, device='cuda')
    raw = out['texture'].view(-1, 3)[out['texel'].long()]
    assert bool((raw == flat).all())                                                  # every covered texel, before the fill
    live = out['region'] != 0                                                         # covered, or within `pad` of a covered texel
    if ssaa == 2:
        live = live.view(size, 2, size, 2).all(dim=3).all(dim=1)
    assert bool((out['normal'][live] == flat).all())
    assert int(live.sum()) > int(out['mask'].sum()) and bool(live[out['mask']].all())  # the gutter is part of it


# ---- 4. the bake, detail ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', ['tangent', 'object'])
def test_the_baked_bytes_equal_the_restatement(TF, source, detail, space):
    out = detail[space]
    sid = R.TANGENT if space == 'tangent' else R.OBJECT
    face, bary = _np(out['face']), _np(out['bary'])
    n = len(face)
    assert out['unmatched'] == 0 and (face >= 0).all() and n == int((out['tri_id'] >= 0).sum()) and 0.02 < out['max_moved'] < 0.08
    ns32 = R.attr_at(source['normals'], source['f'], face, bary)
    assert np.array_equal(_bits(out['source_normals']), _bits(ns32))
    nrm, tan, sign = _np(out['frame_normals']), _np(out['tangents']), _np(out['sign'])
    got = _np(out['texture']).reshape(-1, 3)[_np(out['texel'])]
    want32, bad32 = R.encode(nrm, tan, sign, ns32, face >= 0, sid, np.float32)
    assert not bad32.any() and np.array_equal(got, want32)
    ns64 = R.attr_at(source['normals'], source['f'], face, bary, dtype=np.float64)
    want64, _ = R.encode(nrm, tan, sign, ns64, face >= 0, sid, np.float64)
    gap = np.abs(got.astype(np.int32) - want64.astype(np.int32))
    print(f'{space}: {n} texels, {int((gap > 0).sum())} differ from the float64 restatement, by at most {int(gap.max())} level')
    assert gap.max() <= 1
    if space == 'tangent':                                                            # the detail is there: the map is not flat
        assert (got != R.FLAT).any(1).mean() > 0.5 and got[:, 2].min() > 128
    untouched = torch.ones(out['texture'].shape[:2], dtype=torch.bool, device='cuda').view(-1)
    untouched[out['texel'].long()] = False
    assert not bool(out['texture'].view(-1, 3)[untouched].any())


def test_a_reach_of_two_hundredths_leaves_texels_unmatched(TF, target, source, detail):
    full = detail['tangent']
    out = TF.bake_normal_map(*target, source['tracer'], size=256, ssaa=2, max_dist=0.02, return_intermediates=True)
    face = _np(out['face'])
    assert torch.equal(out['texel'], full['texel'])
    ns32 = R.attr_at(source['normals'], source['f'], face, _np(out['bary']))
    want, bad = R.encode(_np(out['frame_normals']), _np(out['tangents']), _np(out['sign']), ns32, face >= 0, R.TANGENT)
    assert out['unmatched'] == int(bad.sum()) == int((face < 0).sum()) and 0 < out['unmatched'] < len(face)
    got = _np(out['texture']).reshape(-1, 3)[_np(out['texel'])]
    assert np.array_equal(got, want) and (got[face < 0] == R.FLAT).all()
    assert np.array_equal(face < 0, _np(full['dist']) > np.float32(0.02)) and out['max_moved'] <= 0.02
    near = face >= 0
    assert np.array_equal(got[near], _np(full['texture']).reshape(-1, 3)[_np(full['texel'])][near])


def test_baking_the_sources_own_face_normals(TF, target, source):
    """source_normals='face': the hit face's unit normal, turned outward whatever the winding, zeros where nothing is in reach"""
    P = source['v'].astype(np.float64)
    f = source['f']
    fn = np.cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    assert ((fn * P[f].mean(1)).sum(1) > 0).all()                                     # the source is wound outward
    outs = []
    for tris in (f, np.ascontiguousarray(f[:, ::-1])):                                # ... and wound inward: the same normals
        out = TF.bake_normal_map(*target, (source['v'], tris), size=128, ssaa=1, source_normals='face', max_dist=0.03, return_intermediates=True)
        face, ns = _np(out['face']), _np(out['source_normals'])
        hit = face >= 0
        assert 0 < out['unmatched'] == int((~hit).sum()) < len(face) and not ns[~hit].any()
        assert np.abs(ns[hit] - fn[face[hit]]).max() < 1e-6                            # float32 normals of unit length
        want, bad = R.encode(_np(out['frame_normals']), _np(out['tangents']), _np(out['sign']), ns, hit, R.TANGENT)
        got = _np(out['texture']).reshape(-1, 3)[_np(out['texel'])]
        assert np.array_equal(got, want) and np.array_equal(bad, ~hit) and (got[~hit] == R.FLAT).all() and (got[hit] != R.FLAT).any()
        outs.append((face, got))
    # (a reversed triangle is another set of edge vectors to the closest-point function: a texel at the same distance from two faces, or
    # at the edge of the reach, may choose the other; where both windings chose the same face the bytes agree to a level)
    same = outs[0][0] == outs[1][0]
    assert same.mean() > 0.99 and np.abs(outs[0][1][same].astype(np.int32) - outs[1][1][same].astype(np.int32)).max() <= 1
    with pytest.raises(ValueError, match='source_normals'):
        TF.bake_normal_map(*target, source['tracer'], size=64, ssaa=1, source_normals='vertex')


# ---- 5. the lookup ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hits(TF, target, detail):
    """4096 hits on the target with footprints from under a texel to beyond the top level; some miss"""
    from nero_amd import texfetch
    from nero_amd.mesh import vertex_normals
    from nero_amd.surface import sample_surface
    v, f = target
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    out = detail['tangent']
    n = 4096
    _, face, bary = sample_surface(vd, fd, n, seed=3, return_face=True, return_bary=True)
    g = np.random.default_rng(9)
    face = face.clone()
    face[:4] = torch.tensor([-1, len(f), -7, len(f) + 3], dtype=torch.int32, device='cuda')
    depth = torch.from_numpy(np.exp2(g.uniform(-3, 13, n)).astype(np.float32)).cuda()
    normals = vertex_normals(vd, fd, weight='angle', orient='outward')
    nrm_in = TF.attributes_at(normals, fd, face, bary, fill=1.0)
    scale = texfetch.face_scale(vd, fd, out['vt'], out['ft'], 256, 256)
    return dict(v=vd, f=fd, vt=np.asarray(out['vt']), ft=np.asarray(out['ft']), scale=scale, tangent=out['tangent'], sign=out['face_sign'], face=face,
                bary=bary, depth=depth, nrm_in=nrm_in, normals=normals)


def _apply(TF, nm, h, spread, **kw):
    return TF.apply_normal_map(nm, h['vt'], h['ft'], h['scale'], h['tangent'], h['sign'], h['face'], h['bary'], h['depth'], h['nrm_in'], spread, **kw)


def test_a_flat_map_and_a_constant_map(TF, hits):
    flat = TF.NormalMap(np.full((256, 256, 3), R.FLAT, np.uint8))
    assert flat.levels == 9 and all(bool((flat.level(k)[..., :3] == torch.tensor(R.FLAT, dtype=torch.uint8, device='cuda')).all()) and
                                    not bool(flat.level(k)[..., 3].any()) for k in range(9))
    for spread in (None, 0.01, 1.0):
        assert torch.equal(_apply(TF, flat, hits, spread), hits['nrm_in']), spread
    const = TF.NormalMap(np.full((256, 256, 3), (150, 110, 240), np.uint8))
    ok = ((hits['face'] >= 0) & (hits['face'] < hits['f'].shape[0]))
    outs = []
    for spread in (None, 0.01, 1.0):
        out, dbg = _apply(TF, const, hits, spread, return_debug=True)
        outs.append(out)
        assert torch.equal(out[~ok], hits['nrm_in'][~ok]) and not torch.equal(out[ok], hits['nrm_in'][ok])
        if spread == 0.01:
            assert len(set(dbg[ok, 0].tolist())) == 9                                 # every level is visited
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])            # the same vector at every level
    obj = TF.NormalMap(np.full((256, 256, 3), (150, 110, 240), np.uint8), space='object')
    o = _apply(TF, obj, hits, 0.01)
    want = torch.tensor(R.decode(np.asarray([150, 110, 240])), device='cuda')
    nin = hits['nrm_in']
    facing = ok & (((want[0] * nin[:, 0] + want[1] * nin[:, 1]) + want[2] * nin[:, 2]) > 0)          # the kernel's dot product, term by term
    assert bool((o[facing] == want).all()) and torch.equal(o[~facing], hits['nrm_in'][~facing]) and 0 < int(facing.sum()) < int(ok.sum())


@pytest.mark.parametrize('space', ['tangent', 'object'])
def test_the_lookup_equals_the_restatement(TF, hits, detail, space):
    nmap = detail[space]['normal']
    nm = TF.NormalMap(nmap, space=space)
    levels = R.pyramid(_np(nmap))
    assert all(np.array_equal(_np(nm.level(k)), levels[k]) for k in range(nm.levels)) and nm.levels == len(levels) == 9
    h = {k: _np(x) for k, x in hits.items()}
    for spread, bias in ((None, 0.0), (0.01, 0.0), (0.01, -1.5), (1.0, 0.0)):
        got, dbg = _apply(TF, nm, hits, spread, lod_bias=bias, return_debug=True)
        want, wdbg = R.apply(levels, h['vt'], h['ft'], h['scale'], h['tangent'], h['sign'], h['face'], h['bary'], h['depth'], h['nrm_in'],
                             0.0 if spread is None else spread, float(np.exp2(np.float64(bias))), R.TANGENT if space == 'tangent' else R.OBJECT)
        assert np.array_equal(_bits(dbg), _bits(wdbg)), (spread, bias)
        assert np.array_equal(_bits(got), _bits(want)), (spread, bias)
        assert np.array_equal(_bits(got[:4]), _bits(hits['nrm_in'][:4])) and not dbg[:4].any()       # the misses
        if spread == 0.01:
            lv, t = _np(dbg[4:, 0]), _np(dbg[4:, 1])
            assert lv.max() == 8 and lv.min() == 0 and ((t > 0) & (lv < 8)).any() and (t[lv == 8] == 0).all()     # between two levels; the top level
    assert not np.array_equal(_bits(got[4:]), _bits(hits['nrm_in'][4:]))


def test_a_map_that_tilts_past_a_right_angle_falls_back(TF, hits):
    back = TF.NormalMap(np.full((256, 256, 3), (128, 255, 100), np.uint8))            # z below zero
    assert torch.equal(_apply(TF, back, hits, None), hits['nrm_in'])
    edge = TF.NormalMap(np.full((256, 256, 3), (128, 255, 140), np.uint8))            # z above zero: kept
    out = _apply(TF, edge, hits, None)
    ok = ((hits['face'] >= 0) & (hits['face'] < hits['f'].shape[0]))
    assert bool(((out[ok] * hits['nrm_in'][ok]).sum(1) > 0).all()) and not torch.equal(out[ok], hits['nrm_in'][ok])


# ---- 6. the round trip ------------------------------------------------------------------------------------------------------------------------
def test_the_round_trip_brings_the_sources_normals_back(TF, target, source, detail, hits):
    """bake, then look up at 20 000 points of the target at level 0: E_map is the mean angle between the normalised result and the
    source's normal at the point's own closest point (what was baked), E_0 the same for the target's unperturbed normal.  The float64
    restatement makes the same trip from the same closest-point results: the bytes in float64, the integer fill and halving, the
    lookup in float64."""
    from nero_amd import texture as TX
    from nero_amd.surface import sample_surface
    out = detail['tangent']
    vd, fd = hits['v'], hits['f']
    n = 20000
    pts, face, bary = sample_surface(vd, fd, n, seed=11, return_face=True, return_bary=True)
    depth = torch.ones(n, device='cuda')
    nrm_in = TF.attributes_at(hits['normals'], fd, face, bary)
    nm = TF.NormalMap(out['normal'])
    got = TF.apply_normal_map(nm, hits['vt'], hits['ft'], hits['scale'], hits['tangent'], hits['sign'], face, bary, depth, nrm_in)
    _, sface, sbary, _ = source['tracer'].closest(pts)
    truth = R.attr_at(source['normals'], source['f'], _np(sface), _np(sbary), dtype=np.float64)
    E_map = float(R.angle(_np(got), truth).mean())
    E_0 = float(R.angle(_np(nrm_in), truth).mean())
    # the float64 trip
    tface, tbary = _np(out['face']), _np(out['bary'])
    by64, bad = R.encode(_np(out['frame_normals']), _np(out['tangents']), _np(out['sign']),
                         R.attr_at(source['normals'], source['f'], tface, tbary, dtype=np.float64), tface >= 0, R.TANGENT, np.float64)
    tex = torch.zeros_like(out['texture'])
    tex.view(-1, 3)[out['texel'].long()] = torch.from_numpy(by64).cuda()
    map64 = _np(TX.downsample2(TX.fill_gutter(tex, out['region'], 32)))
    nin64 = R.attr_at(_np(hits['normals']), _np(fd), _np(face), _np(bary), dtype=np.float64)
    ref, _ = R.apply(R.pyramid(map64), hits['vt'], hits['ft'], _np(hits['scale']), _np(hits['tangent']), _np(hits['sign']), _np(face), _np(bary),
                     np.ones(n, np.float32), nin64, 0.0, 1.0, R.TANGENT, np.float64)
    E_ref = float(R.angle(ref, truth).mean())
    print(f'round trip: E_0 {np.degrees(E_0):.3f} deg, E_map {np.degrees(E_map):.3f} deg (ratio {E_map / E_0:.3f}), '
          f'float64 restatement {np.degrees(E_ref):.3f} deg, |E_map - E_ref| {abs(E_map - E_ref):.2e} rad')
    assert not bad.any() and np.radians(5.0) < E_0 < np.radians(15.0)         # (the bumps tilt the source's normals by some ten degrees)
    assert abs(E_map - E_ref) <= 1e-4
    assert E_map < E_0
    assert E_map <= 2.0 * E_ref


# ---- 7. the relighter -------------------------------------------------------------------------------------------------------------------------
POSE = RR.relighting_poses(4, 30.0, 60.0, 2.4)[1].numpy()


def _K(side, focal):
    return np.asarray([[focal, 0, side / 2], [0, focal, side / 2], [0, 0, 1]], np.float32)


def _mats(V, seed=None):
    if seed is None:
        return {'metallic': np.full((V, 1), 0.7, np.float32), 'roughness': np.full((V, 1), 0.35, np.float32), 'albedo': np.full((V, 3), 0.8, np.float32)}
    g = np.random.default_rng(seed)
    return {'metallic': g.uniform(0, 1, (V, 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (V, 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (V, 3)).astype(np.float32)}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('textured', [False, True])
@pytest.mark.parametrize('normals', [None, 'angle'])
def test_a_flat_map_renders_the_same_bits(TF, target, textured, normals):
    from nero_amd import relight as RL
    from nero_amd.texture import simple_atlas
    from tests import texfetch_ref as XR
    v, f = target
    vt, ft = simple_atlas(v, f, 64)
    env = RR.proper_map(16, 32, seed=2, hot=(3, 20, 100.0))
    alb, met, rgh = XR.random_maps(64, 64, seed=2)
    kw = dict(textures={'albedo': alb, 'metallic': met, 'roughness': rgh, 'vt': vt, 'ft': ft}, lod_bias=2.0) if textured else {}
    mats = None if textured else _mats(len(v), seed=0)
    plain = RL.Relighter(v, f, mats, env, normals=normals, **kw)
    flat = RL.Relighter(v, f, mats, env, normals=normals, tracer=plain.tracer,
                        normal_map={'normal': np.full((64, 64, 3), R.FLAT, np.uint8), 'vt': vt, 'ft': ft}, **kw)
    assert plain.normal_map is None and flat.normal_map.levels == 7
    for denoise in (False, True):
        a = plain.render(POSE, _K(48, 60.0), 48, 48, samples=(8, 8), denoise=denoise)
        _same(a, flat.render(POSE, _K(48, 60.0), 48, 48, samples=(8, 8), denoise=denoise))
        assert int((a['alpha'] > 0).sum()) > 300
    ro, rd = plain.camera_rays(POSE, _K(48, 60.0), 48, 48)
    assert torch.equal(plain.surface(ro, rd, spread=1 / 60.0)['normal'], flat.surface(ro, rd, spread=1 / 60.0)['normal'])


def _lobe_env(origin):
    """a smooth 16 x 32 map on the project's own grid ('nero' convention): a dim sky and one broad bright lobe, 40 degrees off the
    direction of the camera so that the lit side faces it"""
    d = RR.grid_directions(16, 32, False).numpy()
    c = origin / np.linalg.norm(origin)
    side = np.cross(c, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    lobe = np.cos(np.radians(40.0)) * c + np.sin(np.radians(40.0)) * side
    env = 0.1 + 8.0 * np.exp(3.0 * ((d * lobe).sum(-1) - 1.0))
    env = np.repeat(env[..., None], 3, -1).astype(np.float32)
    env[:, -1] = env[:, 0]
    env[0], env[-1] = env[0].mean(0), env[-1].mean(0)
    return env


def test_the_map_brings_the_render_closer_to_the_dense_mesh(TF, target, source, detail):
    """one pose, one seed, 64 x 64, (64, 64) samples: the source mesh with smooth normals, the target, the target with the baked map.
    On the pixels whose 3 x 3 neighbourhood is hit in all three, the render with the map is closer to the source's."""
    from nero_amd import relight as RL
    v, f = target
    K = _K(64, 110.0)
    probe = RL.Relighter(v, f, _mats(len(v)), np.ones((16, 32, 3), np.float32), convention='nero', normals='angle')
    origin = probe.camera_rays(POSE, K, 64, 64)[0][0].cpu().numpy().astype(np.float64)
    env = _lobe_env(origin)
    out = detail['tangent']
    nmap = {'normal': out['normal'], 'vt': out['vt'], 'ft': out['ft'], 'space': 'tangent'}
    rl_src = RL.Relighter(source['v'], source['f'], _mats(len(source['v'])), env, convention='nero', normals='angle', tracer=source['tracer'])
    rl_tgt = RL.Relighter(v, f, _mats(len(v)), env, convention='nero', normals='angle', tracer=probe.tracer)
    rl_map = RL.Relighter(v, f, _mats(len(v)), env, convention='nero', normals='angle', tracer=probe.tracer, normal_map=nmap)
    pics = [r.render(POSE, K, 64, 64, samples=(64, 64), seed=5) for r in (rl_src, rl_tgt, rl_map)]
    hit = torch.stack([p['alpha'][..., 0] > 0 for p in pics]).all(0).float()
    inner = torch.nn.functional.avg_pool2d(hit[None, None], 3, 1, 1)[0, 0] > 0.999
    assert int(inner.sum()) > 1000
    rmse = lambda a, b: float(((a['rgb_lin'][inner] - b['rgb_lin'][inner]) ** 2).mean().sqrt())
    e_tgt, e_map = rmse(pics[1], pics[0]), rmse(pics[2], pics[0])
    level = float(pics[0]['rgb_lin'][inner].mean())
    print(f'relit: RMSE(target, source) {e_tgt:.4f}, RMSE(target + map, source) {e_map:.4f}, mean radiance {level:.4f}, {int(inner.sum())} pixels')
    assert e_map < e_tgt
    nerr = lambda p: float(R.angle(_np(p['normal'][inner]), _np(pics[0]['normal'][inner])).mean())
    assert nerr(pics[2]) < nerr(pics[1])                                              # the normals the estimator saw


def test_the_asset_with_a_normal_map_round_trips(TF, target, detail, tmp_path):
    from nero_amd import relight as RL
    from nero_amd.texture import read_textured_obj, write_textured_obj
    from tests import texfetch_ref as XR
    v, f = target
    out = detail['tangent']
    alb, met, rgh = XR.random_maps(256, 256, seed=4)
    maps = {'albedo': alb, 'metallic': met, 'roughness': rgh, 'vt': out['vt'], 'ft': out['ft']}
    env = RR.proper_map(16, 32, seed=2, hot=(3, 20, 100.0))
    nmap = {k: out[k] for k in ('normal', 'vt', 'ft', 'space')}
    rl = RL.Relighter(v, f, None, env, textures=maps, normal_map=nmap, normals='angle')
    obj = write_textured_obj(str(tmp_path), v, f, out['vt'], out['ft'], {**maps, 'normal': out['normal'], 'space': out['space'], 'normals': out['normals']})
    back = read_textured_obj(obj)
    assert np.array_equal(back['normal'], _np(out['normal'])) and back['normal_space'] == 'tangent' and back['normal_frame'] == 'angle'
    assert np.array_equal(back['vt'], out['vt'])
    again = RL.Relighter.from_asset(obj, env)
    assert again._computed_normals and torch.equal(again.normals, rl.normals) and torch.equal(again.normal_map.pyramid, rl.normal_map.pyramid)
    assert torch.equal(again.nm_tangent, rl.nm_tangent) and torch.equal(again.nm_sign, rl.nm_sign)
    K = _K(48, 60.0)
    pic = rl.render(POSE, K, 48, 48, samples=(8, 8))
    _same(pic, again.render(POSE, K, 48, 48, samples=(8, 8)))
    bare = RL.Relighter.from_asset(obj, env, normal_map=None, normals='angle')
    assert bare.normal_map is None and not torch.equal(bare.render(POSE, K, 48, 48, samples=(8, 8))['normal'], pic['normal'])


# ---- 8. the asset of a simplified mesh --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    from nero_amd.renderer import NeROMaterialRenderer
    from tests.helpers import build_material_case, golden_mesh, load_golden
    _, meta = load_golden('mat_bell')
    ref = build_material_case(meta)
    net = NeROMaterialRenderer({'shader_cfg': meta['shader_cfg'], 'database_name': 'syn/bell'}, mesh=golden_mesh())
    net.load_state_dict(ref.state_dict())
    return net.cuda()


def test_bake_asset_on_the_renderers_own_mesh_and_on_a_simplified_one(TF, net):
    from nero_amd import texture as TX
    own = TF.bake_asset(net, size=128)
    assert own['unmatched'] == 0 and own['max_moved'] < 1e-6 and own['tris'].shape[0] == net.mesh_triangles.shape[0]
    base = TX.bake_materials(net, vt=own['vt'], ft=own['ft'], size=128)
    assert torch.equal(own['mask'], base['mask'])
    for k in ('albedo', 'metallic', 'roughness'):
        gap = (own[k][own['mask']].int() - base[k][base['mask']].int()).abs()
        print(f'{k}: projected against unprojected points, {int((gap > 0).sum())} of {gap.numel()} bytes differ, by at most {int(gap.max())}')
        assert int(gap.max()) <= 1 and tuple(own[k].shape[:2]) == (128, 128)
    flat = torch.tensor(R.FLAT, dtype=torch.uint8, device='cuda')
    assert tuple(own['normal'].shape) == (128, 128, 3) and bool((own['normal'][own['mask']] == flat).all())
    low = TF.bake_asset(net, target_faces=600, size=128)
    assert 100 < low['tris'].shape[0] <= 600 and low['unmatched'] == 0 and 0 < low['max_moved'] < 0.1
    assert all(tuple(low[k].shape[:2]) == (128, 128) for k in ('albedo', 'metallic', 'roughness', 'normal', 'mask'))
    assert low['space'] == 'tangent' and low['normals'] == 'angle' and low['ft'].shape[0] == low['tris'].shape[0]
    assert not bool((low['normal'][low['mask']] == flat).all())
    again = TF.bake_asset(net, target_faces=600, size=128)
    for k in ('albedo', 'metallic', 'roughness', 'normal', 'mask', 'verts', 'tris'):
        assert torch.equal(low[k], again[k]), k


# ---- 9. the scripts ---------------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'scripts'))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def test_the_scripts_bake_and_relight_a_simplified_asset(TF, tmp_path, capsys):
    import json
    from nero_amd import relight as RL
    from nero_amd.envlight import write_hdr
    from nero_amd.mesh import write_ply
    from nero_amd.texture import read_png, read_textured_obj
    from tests.helpers import golden_mesh
    v, f = golden_mesh()
    ply, out = str(tmp_path / 'mesh.ply'), str(tmp_path / 'asset')
    write_ply(ply, v, f)
    _script('extract_texture_maps').main(['--mesh', ply, '--target-faces', '600', '--atlas', 'charts', '--normal-map', '--size', '128', '--out', out,
                                          '--name', 'mesh_3'])
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 100 < report['triangles'] <= 600 and report['source_triangles'] == len(f) and report['normal_map'] and report['unmatched'] == 0
    assert report['normal_space'] == 'tangent' and report['normals'] == 'angle' and report['atlas'] == 'chart_atlas'
    back = read_textured_obj(report['obj'])
    assert len(back['f']) == report['triangles'] and back['norm'] == 'feat4_3.png' and back['normal_frame'] == 'angle'
    assert back['normal'].shape == (128, 128, 3) and (back['normal'] != R.FLAT).any()
    hdr = str(tmp_path / 'e.hdr')
    write_hdr(hdr, RR.proper_map(8, 16, seed=6).numpy())
    relight = _script('relight')
    common = ['--mesh', report['obj'], '--textured', '--hdr', hdr, '--out', str(tmp_path / 'out'), '--num', '1', '--width', '32', '--height', '32',
              '--samples', '8', '8', '--cam_dist', '2.0']
    relight.main(common + ['--name', 'with'])
    relight.main(common + ['--name', 'without', '--no-normal-map'])
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(1, 0.0, 30.0, 2.0))[0]
    pics = {}
    for name, kw in (('with', {}), ('without', {'normal_map': None})):
        pics[name] = read_png(str(tmp_path / 'out' / name / '0.png'))
        rl = RL.Relighter.from_asset(report['obj'], hdr, **kw)
        assert (rl.normal_map is not None) == (name == 'with') and rl._computed_normals == (name == 'with')
        assert np.array_equal(pics[name], rl.render(pose, RL.default_K(32, 32), 32, 32, samples=(8, 8))['rgba8'].cpu().numpy()), name
    assert not np.array_equal(pics['with'], pics['without']) and int((pics['with'][..., 3] > 0).sum()) > 50
    with pytest.raises(SystemExit):
        relight.main(['--mesh', ply, '--material', 'x', '--hdr', hdr, '--name', 'n', '--no-normal-map'])
    # an asset whose tangent-space map was baked in the caller's own frame normals: refused, as Relighter.from_asset refuses it
    mtl = report['obj'][:-4] + '.mtl'
    text = open(mtl).read()
    assert 'normals=angle' in text
    open(mtl, 'w').write(text.replace('normals=angle', 'normals=custom'))
    with pytest.raises(SystemExit, match='normals=custom'):
        relight.main(common + ['--name', 'custom'])
    with pytest.raises(ValueError, match='own normals'):
        RL.Relighter.from_asset(report['obj'], hdr)
    relight.main(common + ['--name', 'custom_off', '--no-normal-map'])
    assert np.array_equal(read_png(str(tmp_path / 'out' / 'custom_off' / '0.png')), pics['without'])
    # --gutter reaches the chart atlas of the transfer path
    wide = str(tmp_path / 'wide')
    _script('extract_texture_maps').main(['--mesh', ply, '--target-faces', '600', '--atlas', 'charts', '--gutter', '8', '--normal-map', '--size', '128',
                                          '--out', wide, '--name', 'mesh_3'])
    rep8 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep8['triangles'] == report['triangles'] and rep8['covered_texels'] < report['covered_texels']
