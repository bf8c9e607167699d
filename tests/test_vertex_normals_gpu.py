"""GPU tier: the vertex-normal kernels (nero_amd/csrc/mesh_normals.hip through nero_amd.mesh.vertex_normals) against the numpy restatement
tests/normals_ref.py (pinned by tests/test_vertex_normals_cpu.py).  AREA mode BIT FOR BIT, normals and info: the contract rounds every
float64 operation on its own, the kernels are built without contraction, the sums are integers.  ANGLE mode within 2^-23 per component and
with equal info: the device's float64 atan2 may differ from numpy's in its last places, which moves a fixed-point term by at most one unit of
2^-B; a vertex's sum is then perturbed far below half an fp32 ulp except at a rounding tie, so a component differs by at most one fp32 ulp,
<= 2^-24 below 1.  Then the relighter over computed normals against the same normals passed as a tensor, bit for bit."""
import numpy as np
import pytest
import torch

from tests import normals_ref as NR
from tests import relight_ref as RR

pytestmark = pytest.mark.gpu

MODES = ('area', 'angle')
MESHES = ('one_triangle', 'one_vertex', 'icosphere', 'icosphere_small', 'icosphere_large', 'fan', 'grid257', 'grid65537', 'spoiled')
POSE = RR.relighting_poses(4, 30.0, 60.0, 2.4)[1].numpy()
KMAT = np.asarray([[60.0, 0, 24], [0, 60.0, 24], [0, 0, 1]], np.float32)


@pytest.fixture(scope='module')
def M():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import mesh
    return mesh


@pytest.fixture(scope='module')
def RL(M):
    from nero_amd import relight
    return relight


def _icosphere(*a, **kw):
    from nero_amd.synthetic import icosphere
    return icosphere(*a, **kw)


def _mesh(name):
    if name == 'one_triangle':
        return np.asarray([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.7, 0.9]], np.float32), np.asarray([[0, 1, 2]], np.int32)
    if name == 'one_vertex':
        return np.asarray([[0.5, 0.25, 2.0]], np.float32), np.asarray([[0, 0, 0]], np.int32)
    if name.startswith('icosphere'):
        v, f = _icosphere(3, 0.5, bumps=0.05)
        scale = {'icosphere': 1.0, 'icosphere_small': 1e-6, 'icosphere_large': 1e6}[name]
        return (v * np.float32(scale)).astype(np.float32), f
    if name == 'fan':
        return NR.fan(4096)
    if name.startswith('grid'):
        return NR.grid(int(name[4:]))
    v, f = _icosphere(3, 0.5, bumps=0.05)
    return NR.spoiled(v, f)[:2]


@pytest.fixture(scope='module')
def cases(M):
    """every mesh once: the restatement in both modes, and the device's answer in both modes"""
    out = {}
    for name in MESHES:
        v, f = _mesh(name)
        ref = {w: NR.vertex_normals(v, f, w) for w in MODES}
        dev = {}
        for w in MODES:
            n, info = M.vertex_normals(v, f, weight=w, return_info=True)
            assert n.is_cuda and n.dtype == torch.float32 and tuple(n.shape) == (len(v), 3) and info.is_cuda and info.dtype == torch.int64
            dev[w] = (n.cpu().numpy(), info.cpu().numpy())
        out[name] = (v, f, ref, dev)
    return out


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. against the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MESHES)
def test_area_mode_has_the_restatement_s_bits(cases, name):
    v, f, ref, dev = cases[name]
    (n_ref, info_ref), (n, info) = ref['area'], dev['area']
    assert np.array_equal(info, info_ref), (info, info_ref)
    assert np.array_equal(_bits(n), _bits(n_ref)), int((_bits(n) != _bits(n_ref)).sum())
    if name == 'one_vertex':
        assert info.tolist() == [0, 1, 1, 0] and not n.any()
    if name == 'fan':                                                  # the largest sums: 4096 terms on one vertex
        assert int(np.abs(NR.vertex_sums(v, f, 'area')[0][0]).max()) > 2 ** 50
    if name in ('icosphere_small', 'icosphere_large'):                 # the exponent moved with the scale, the normals did not move far
        assert abs(int(info[3]) - int(cases['icosphere'][3]['area'][1][3])) >= 38
        assert np.abs(n - cases['icosphere'][3]['area'][0]).max() < 1e-5


@pytest.mark.parametrize('name', MESHES)
def test_angle_mode_is_within_an_ulp_of_the_restatement(cases, name):
    v, f, ref, dev = cases[name]
    (n_ref, info_ref), (n, info) = ref['angle'], dev['angle']
    assert np.array_equal(info, info_ref), (info, info_ref)
    assert info[3] == 0
    err = float(np.abs(n.astype(np.float64) - n_ref.astype(np.float64)).max())
    differ = float((_bits(n) != _bits(n_ref)).mean())
    print(f'angle mode on {name}: largest difference {err:.3e} (bound 2^-23 = {2.0 ** -23:.3e}), {differ:.4%} of {n.size} components differ in their bits')
    assert err <= 2.0 ** -23


def test_spoiled_entries_contribute_nothing(cases):
    """an out-of-range index, a negative one, a NaN vertex used by two faces, an unreferenced vertex and a repeated index: the vertices of
    the clean mesh keep its bits, the two added vertices are zero, the counters are right"""
    v, f = _icosphere(3, 0.5, bumps=0.05)
    keep = NR.spoiled(v, f)[2]
    for w in MODES:
        n_clean, info_clean = cases['icosphere'][3][w]
        n, info = cases['spoiled'][3][w]
        assert np.array_equal(_bits(n[keep]), _bits(n_clean))
        assert not n[len(v):].any()
        assert info[:3].tolist() == [4, 1, 2] and info[3] == info_clean[3]


# ---- 2. the same bits, whatever the schedule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weight', MODES)
def test_runs_orders_and_streams_give_the_same_bits(M, cases, weight):
    for name in ('icosphere', 'fan', 'grid65537'):
        v, f, _, dev = cases[name]
        first = dev[weight][0]
        vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        again = M.vertex_normals(vd, fd, weight=weight)
        assert again.device == vd.device and np.array_equal(_bits(again.cpu().numpy()), _bits(first))
        perm = torch.from_numpy(np.random.default_rng(7).permutation(len(f))).cuda()
        shuffled, info = M.vertex_normals(vd, fd[perm], weight=weight, return_info=True)
        assert np.array_equal(_bits(shuffled.cpu().numpy()), _bits(first)) and np.array_equal(info.cpu().numpy(), dev[weight][1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = M.vertex_normals(vd, fd, weight=weight)
        side.synchronize()
        assert np.array_equal(_bits(on_side.cpu().numpy()), _bits(first))


@pytest.mark.parametrize('weight', MODES)
def test_outward_orientation_undoes_a_reversed_winding(M, cases, weight):
    v, f, _, dev = cases['icosphere']
    rev = np.ascontiguousarray(f[:, ::-1])
    assert M.winding_sign(v, f) == 1 and M.winding_sign(torch.from_numpy(v).cuda(), torch.from_numpy(rev).cuda()) == -1
    out = M.vertex_normals(v, f, weight=weight, orient='outward').cpu().numpy()
    out_rev = M.vertex_normals(v, rev, weight=weight, orient='outward').cpu().numpy()
    assert np.array_equal(_bits(out), _bits(dev[weight][0])) and np.array_equal(_bits(out_rev), _bits(out))
    as_wound = M.vertex_normals(v, rev, weight=weight).cpu().numpy()
    assert np.array_equal(as_wound, -out) and float((as_wound * v).sum(1).max()) < 0
    sheet = M.vertex_normals(*_mesh('one_triangle'), weight=weight, orient='outward').cpu().numpy()          # no volume: no outside
    assert not sheet.any() and not np.signbit(sheet).any()


# ---- 3. the relighter -----------------------------------------------------------------------------------------------------------------------
def _materials(nV, seed=0):
    g = np.random.default_rng(seed)
    return {'metallic': g.uniform(0, 1, (nV, 1)).astype(np.float32), 'roughness': g.uniform(0.2, 0.9, (nV, 1)).astype(np.float32),
            'albedo': g.uniform(0.1, 0.9, (nV, 3)).astype(np.float32)}


def _render(rl, **kw):
    return rl.render(POSE, KMAT, 48, 48, samples=(16, 16), **kw)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope='module')
def bumpy(RL):
    v, f = _icosphere(3, 0.5, bumps=0.05)
    return v, f, _materials(len(v)), RR.proper_map(16, 32, seed=2, hot=(3, 20, 100.0))


@pytest.mark.parametrize('reverse', [False, True])
def test_computed_normals_render_as_the_same_normals_passed_in(M, RL, bumpy, reverse):
    v, f, mats, env = bumpy
    faces = np.ascontiguousarray(f[:, ::-1]) if reverse else f
    rl = RL.Relighter(v, faces, mats, env, normals='area')
    want = NR.vertex_normals(v, f, 'area')[0]                           # outward: the restatement on the outward winding
    assert rl.normals.is_cuda and np.array_equal(_bits(rl.normals.cpu().numpy()), _bits(want))
    passed = RL.Relighter(v, faces, mats, env, normals=M.vertex_normals(v, faces, 'area', orient='outward'))
    a, b = _render(rl), _render(passed)
    _same(a, b)
    assert float(a['alpha'].sum()) > 100 and float(a['rgb_lin'].max()) > 0
    _same(_render(rl, bounces=1), _render(passed, bounces=1))
    angle = RL.Relighter(v, faces, mats, env, normals='angle', bounces=1)
    _same(_render(angle), _render(RL.Relighter(v, faces, mats, env, normals=angle.normals), bounces=1))
    with pytest.raises(ValueError, match='normals'):
        RL.Relighter(v, faces, mats, env, normals='smooth')


def _surface_normal_as_before(RL, rl, rays_o, rays_d):
    """the lines of Relighter.surface before computed normals existed, on the same hits"""
    _, face, bary = RL.trace_faces(rl.tracer, rays_o, rays_d)
    idx = torch.nonzero(face >= 0)[:, 0]
    f = rl.tris[face[idx].long()]
    u, v = bary[idx, 0:1], bary[idx, 1:2]
    wts = torch.stack([1.0 - u - v, u, v], 1)
    corner = rl.verts[f]
    if rl.normals is None:
        nrm = torch.linalg.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0])
        nrm = torch.where((nrm * rays_d[idx]).sum(-1, keepdim=True) > 0, -nrm, nrm)
    else:
        nrm = (wts * rl.normals[f]).sum(1)
    return torch.nn.functional.normalize(nrm, dim=-1)


def test_flat_and_passed_normals_keep_their_bits(M, RL, bumpy):
    """normals=None and normals=[V,3] against a twin built with the old keyword set only (no `normals` at all for the flat one), and the
    shading normal of both against the arithmetic surface() used before"""
    v, f, mats, env = bumpy
    flat, twin = RL.Relighter(v, f, mats, env, normals=None), RL.Relighter(v, f, mats, env)
    _same(_render(flat), _render(twin))
    _same(_render(flat, bounces=1), _render(twin, bounces=1))
    mine = torch.nn.functional.normalize(torch.from_numpy(np.random.default_rng(3).normal(size=v.shape).astype(np.float32)), dim=-1)
    mine[5] = 0.0                                                       # a caller's own normals are taken as they are, zeros too
    given = RL.Relighter(v, f, mats, env, normals=mine)
    assert torch.equal(given.normals.cpu(), mine)
    for rl in (flat, given):
        ro, rd = rl.camera_rays(POSE, KMAT, 48, 48)
        sf = rl.surface(ro, rd)
        before = _surface_normal_as_before(RL, rl, ro, rd)
        assert sf['normal'].shape == before.shape and before.shape[0] > 100
        assert torch.equal(sf['normal'].view(torch.int32), before.view(torch.int32))


def test_zero_normals_fall_back_to_the_flat_normal(M, RL, bumpy):
    """computed modes only: where the interpolated normal has no direction the camera-facing flat normal stands in"""
    v, f, mats, env = bumpy
    rl = RL.Relighter(v, f, mats, env, normals='angle')
    flat = RL.Relighter(v, f, mats, env, tracer=rl.tracer)
    ro, rd = rl.camera_rays(POSE, KMAT, 48, 48)
    smooth, want = rl.surface(ro, rd)['normal'], flat.surface(ro, rd)['normal']
    rl.normals = torch.zeros_like(rl.normals)
    assert torch.equal(rl.surface(ro, rd)['normal'], want) and not torch.equal(smooth, want)
    rl.normals = torch.full_like(rl.normals, float('nan'))
    assert torch.equal(rl.surface(ro, rd)['normal'], want)


def test_smooth_normals_of_a_sphere_render_radial(RL):
    """the 'normal' plane of icosphere(3, 0.5): with normals='angle' within 0.35 degrees of the radial direction at every hit pixel (the
    vertices' worst is 0.299, tests/test_vertex_normals_cpu.py, and a point of a face and its interpolated normal are the same convex
    combination of the corners' radii and normals), while the flat render's worst pixel is beyond 2 (the corners' worst is 5.45)"""
    v, f = _icosphere(3, 0.5)
    mats, env = _materials(len(v)), RR.proper_map(16, 32, seed=2)
    worst = {}
    for mode in ('angle', None):
        rl = RL.Relighter(v, f, mats, env, normals=mode)
        plane = _render(rl)['normal'].reshape(-1, 3)
        sf = rl.surface(*rl.camera_rays(POSE, KMAT, 48, 48))
        assert sf['idx'].numel() > 100
        radial = torch.nn.functional.normalize(sf['pts'].double(), dim=-1).cpu().numpy()
        worst[mode] = NR.worst_angle_deg(plane[sf['idx']].double().cpu().numpy(), radial)
    print('worst angle to the radius over the hit pixels: smooth', worst['angle'], 'flat', worst[None])
    assert worst['angle'] < 0.35 and worst[None] > 2.0


# ---- 4. the command lines -------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('_normals_cli_' + name, os.path.join(root, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_command_lines(tmp_path, M, RL):
    """extract_mesh.py --in ... --normals writes outward normals of the mesh it writes (here: wound inwards, as extract_mesh.py's own are);
    relight.py --normals angle renders what Relighter(normals='angle') renders, and without the flag what it always rendered"""
    import os
    from nero_amd.envlight import write_hdr
    from nero_amd.texture import read_png
    v, f = _icosphere(2, 0.5, bumps=0.05)
    inward = np.ascontiguousarray(f[:, ::-1])
    src, dst = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply')
    M.write_ply(src, v, inward)
    out = _script('extract_mesh').main(['--in', src, '--normals', 'area', '--out', dst])
    assert out['normals'] == {'weight': 'area', 'refused_faces': 0, 'faces_without_area': 0, 'zero_normals': 0}
    v2, f2, n2 = M.read_ply(dst, with_normals=True)
    assert np.array_equal(v2.astype(np.float32), v) and np.array_equal(f2, inward)
    assert np.array_equal(_bits(n2), _bits(NR.vertex_normals(v, f, 'area')[0])) and float((n2 * v).sum(1).min()) > 0
    _script('extract_mesh').main(['--in', src, '--out', dst])
    assert M.read_ply(dst, with_normals=True)[2] is None
    mats = _materials(len(v), 2)
    os.makedirs(tmp_path / 'mat')
    for k, a in mats.items():
        np.save(tmp_path / 'mat' / f'{k}.npy', a)
    write_hdr(str(tmp_path / 'e.hdr'), RR.proper_map(8, 16, seed=6).numpy())
    pose = RL.poses_in_mesh_frame(RL.relighting_poses(1, 0.0, 30.0, 2.0))[0]
    for flag, mode in (([], None), (['--normals', 'flat'], None), (['--normals', 'angle'], 'angle'), (['--normals', 'area'], 'area')):
        _script('relight').main(['--mesh', src, '--material', str(tmp_path / 'mat'), '--hdr', str(tmp_path / 'e.hdr'), '--name', 'o', '--out',
                                 str(tmp_path / 'r'), '--num', '1', '--width', '32', '--height', '32', '--samples', '16', '16', '--cam_dist', '2.0'] + flag)
        want = RL.Relighter(v, inward, mats, str(tmp_path / 'e.hdr'), normals=mode).render(pose, RL.default_K(32, 32), 32, 32, samples=(16, 16))
        img = read_png(str(tmp_path / 'r' / 'o' / '0.png'))
        assert np.array_equal(img, want['rgba8'].cpu().numpy()) and 50 < int((img[..., 3] > 0).sum()) < 1000
