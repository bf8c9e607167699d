"""CPU tier: host-side logic of the drop-in renderers against vectors dumped from the UNMODIFIED reference
(oracle/gen_golden_r2.py -> tests/golden/pools.npz, ref_state.json; oracle/gen_golden.py -> the render cases):
a1 helpers (get_human_coordinate_poses, _process_ray_batch, near_far_from_sphere; network/renderer.py:230-272), the Stage-I ray
pool (network/renderer.py:167-187), the state_dict surface, and the C restatement of the tracer oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pools():
    return np.load(os.path.join(GOLDEN, 'pools.npz'))


def _shape_net(cfg=None):
    from nero_amd.renderer import NeROShapeRenderer
    torch.manual_seed(0)
    return NeROShapeRenderer(cfg or {}, training=False)


def test_human_coordinate_poses_vs_reference():
    z = _pools()
    net = _shape_net()
    poses = torch.from_numpy(z['poses'])
    assert np.abs(net.get_human_coordinate_poses(poses).numpy() - z['human_poses_img']).max() < 1e-6
    assert np.abs(_shape_net({'fixed_camera': True}).get_human_coordinate_poses(poses).numpy() - z['human_poses_img_fixed']).max() < 1e-6
    assert torch.equal(poses, torch.from_numpy(z['poses']))                      # the input is not modified
    # and the per-ray frames stored with every render case
    for name in ('bell_s25000', 'bear_s25000', 'bell_val'):
        g, _ = load_golden(name)
        if 'poses_img' in g.files:
            hp = net.get_human_coordinate_poses(torch.from_numpy(g['poses_img']))
            assert np.abs(hp.numpy() - g['human_poses']).max() < 1e-6, name


def test_process_ray_batch_vs_reference():
    z = _pools()
    net = _shape_net()
    sel = torch.from_numpy(z['s1/sel'])
    batch = {'dirs': torch.from_numpy(z['s1/dirs'])[sel], 'idxs': torch.from_numpy(z['s1/idxs'])[sel]}      # idxs [n,1] like the reference
    poses = torch.from_numpy(z['poses'])
    ro, rd, near, far, hp = net._process_ray_batch(batch, poses)
    for got, key in ((ro, 'rays_o'), (rd, 'rays_d'), (near, 'near'), (far, 'far'), (hp, 'human_poses')):
        assert got.shape == z['s1/' + key].shape, key
        assert np.abs(got.numpy() - z['s1/' + key]).max() < 2e-6, key
    # cached per-image frames give the same answer
    hp2 = net._process_ray_batch(batch, poses, net.get_human_coordinate_poses(poses))[4]
    assert torch.equal(hp, hp2)


# ---- cached state: the camera centres must follow the pose tensor they are asked for, whatever was asked before -------------
def _views(n):
    from nero_amd.synthetic import look_at_pose
    cams = ([3.0, 0.2, 0.5], [-0.4, 2.6, 1.1], [-1.9, -2.1, 1.6], [0.3, -3.2, -0.8], [2.2, 2.0, 0.4], [-2.8, 0.5, -0.6])
    return [torch.from_numpy(look_at_pose(np.array(c, dtype=np.float64))) for c in cams[:n]]


def _ray_batch(n_img, n=37, seed=4):
    g = torch.Generator().manual_seed(seed)
    return {'dirs': torch.randn(n, 3, generator=g), 'idxs': torch.randint(0, n_img, (n,), generator=g)}


def _assert_rays_of(got, poses, batch, where):
    """rays_o within the derived fp32 bound of the float64 centres of `poses` [imn,3,4]; all five outputs equal a fresh renderer's"""
    from tests.helpers import centre_bound
    idx = batch['idxs'].numpy()
    cb = [centre_bound(p) for p in poses]
    want, bound = np.stack([cb[i][0] for i in idx]), np.stack([cb[i][1] for i in idx])
    err = np.abs(got[0].numpy().astype(np.float64) - want)
    assert (err <= bound).all(), (where, float((err / bound).max()))
    fresh = _shape_net()._process_ray_batch(batch, poses.clone())
    for a, b, k in zip(got, fresh, ('rays_o', 'rays_d', 'near', 'far', 'human_poses')):
        assert torch.equal(a, b), (where, k)


def test_camera_centres_after_another_pose_at_the_same_address():
    """A pose tensor whose address, version counter and shape equal those of the previous call's -- what the caching allocator hands out
    when render_image's [1,3,4] pose is released and the next view allocates its own -- reproduced without the allocator: a DLPack alias
    shares the memory and has a version counter of its own, so a pose written through it leaves (data_ptr, _version, shape) of the
    original untouched.  rays_o must be the centre of the pose that is THERE: float64 -R^T t to 4 * 2^-24 * sum_j |R_ji| |t_j| (a
    three-term fp32 dot product, gamma_3 rounded up; tests.helpers.centre_bound), and every output a fresh renderer's."""
    from torch.utils.dlpack import from_dlpack, to_dlpack
    net = _shape_net()
    P1, P2, P3 = _views(3)
    batch = _ray_batch(1)
    A = P1.clone().reshape(1, 3, 4)
    alias = from_dlpack(to_dlpack(A))
    key = lambda t: (t.data_ptr(), t._version, tuple(t.shape))
    k0 = key(A)
    _assert_rays_of(net._process_ray_batch(batch, A), P1.reshape(1, 3, 4), batch, 'first pose')
    alias.copy_(P2.reshape(1, 3, 4))
    assert key(A) == k0 and torch.equal(A[0], P2)                    # same address, same version, same shape -- another camera
    assert float((P2 - P1).abs().max()) > 0.5
    _assert_rays_of(net._process_ray_batch(batch, A), P2.reshape(1, 3, 4), batch, 'second pose through the alias')
    # ... and as the allocator does it: a NEW tensor object on that memory, version 0
    alias.copy_(P3.reshape(1, 3, 4))
    B = from_dlpack(to_dlpack(A))
    assert B is not A and key(B) == k0
    _assert_rays_of(net._process_ray_batch(batch, B), P3.reshape(1, 3, 4), batch, 'third pose, a new tensor on the same memory')


@pytest.mark.parametrize('imn', [3, 1])
def test_camera_centres_over_released_and_new_pose_tensors(imn):
    """pose A, released, then pose B (whatever address the allocator gives it), for a pool of three images and for render_image's [1,3,4];
    then a tensor of another shape at the address of the one before"""
    net = _shape_net()
    V = _views(6)
    batch = _ray_batch(imn)
    A = torch.stack(V[:imn]).clone()
    _assert_rays_of(net._process_ray_batch(batch, A), torch.stack(V[:imn]), batch, 'A')
    del A
    B = torch.stack(V[3:3 + imn]).clone()
    _assert_rays_of(net._process_ray_batch(batch, B), torch.stack(V[3:3 + imn]), batch, 'B after A was released')
    # the same address with another shape: [3,3,4] whose first image is V[5], then its [1,3,4] head
    C3 = torch.stack([V[5], V[0], V[1]]).clone()
    b3, b1 = _ray_batch(3, seed=6), _ray_batch(1, seed=6)
    _assert_rays_of(net._process_ray_batch(b3, C3), C3.clone(), b3, 'three images')
    head = C3[:1]
    assert head.data_ptr() == C3.data_ptr() and head.shape != C3.shape
    _assert_rays_of(net._process_ray_batch(b1, head), C3[:1].clone(), b1, 'one image at the same address')


def test_training_pool_centres_are_cached_on_the_pose_tensor_itself():
    """train_step keeps its saving -- the centres of self.train_poses are computed once per pool, not per step -- and the cache is bound
    to that tensor OBJECT and its version: a second set_ray_pool (the first pool's tensors released, as a caller would) or an in-place
    update of train_poses gives the new centres.  render is replaced by a recorder: this is about the rays it is handed."""
    from tests.helpers import centre_bound
    net = _shape_net({'train_ray_num': 64})
    V = _views(6)
    imgs, Ks = torch.rand(3, 6, 5, 3), torch.tensor([[8.0, 0, 2.5], [0, 8.0, 3.0], [0, 0, 1]]).repeat(3, 1, 1)
    seen = []
    net.render = lambda rays_o, *a, **k: seen.append(rays_o.clone()) or {'ray_rgb': torch.zeros(rays_o.shape[0], 3)}

    def step_and_check(poses, where):
        i0 = net.train_batch_i
        idxs = net.train_batch['idxs'][i0:i0 + 64].numpy()
        net.train_step(25000)
        cb = [centre_bound(p) for p in poses]
        err = np.abs(seen[-1].numpy().astype(np.float64) - np.stack([cb[i][0] for i in idxs]))
        assert (err <= np.stack([cb[i][1] for i in idxs])).all(), where

    P1 = torch.stack(V[:3]).clone()
    net.set_ray_pool(imgs, Ks, P1, device='cpu')
    step_and_check(torch.stack(V[:3]), 'first pool')
    held = net._train_cam_centres()
    step_and_check(torch.stack(V[:3]), 'first pool, second step')
    assert net._train_cam_centres() is held                              # not recomputed per step
    del P1, held
    P2 = torch.stack(V[3:]).clone()
    net.set_ray_pool(imgs, Ks, P2, device='cpu')
    step_and_check(torch.stack(V[3:]), 'second pool')
    with torch.no_grad():
        net.train_poses.copy_(torch.stack([V[1], V[4], V[2]]))           # in place: the version counter moves
    step_and_check(torch.stack([V[1], V[4], V[2]]), 'poses updated in place')
    assert net._cam_centres[0] is net.train_poses                        # the cache holds what it was computed from


def test_stage1_pool_contents_vs_reference_construct_ray_batch():
    """set_ray_pool (device-side pool build) == NeROShapeRenderer._construct_ray_batch of the reference, before the shuffle"""
    z = _pools()
    net = _shape_net()
    net._shuffle_train_batch = lambda: setattr(net, 'train_batch_i', 0)           # keep construction order
    net.set_ray_pool(torch.from_numpy(z['imgs']), torch.from_numpy(z['Ks']), torch.from_numpy(z['poses']), device='cpu')
    assert net.tbn == z['s1/dirs'].shape[0]
    assert np.abs(net.train_batch['dirs'].numpy() - z['s1/dirs']).max() < 2e-6
    assert np.array_equal(net.train_batch['rgbs'].numpy(), z['s1/rgbs'])
    assert np.array_equal(net.train_batch['idxs'].numpy(), z['s1/idxs'][:, 0])
    assert np.abs(net._train_human_poses.numpy() - z['human_poses_img']).max() < 1e-6


def test_shuffle_is_a_permutation_and_epoch_wraps():
    z = _pools()
    net = _shape_net({'train_ray_num': 100})
    net.set_ray_pool(torch.from_numpy(z['imgs']), torch.from_numpy(z['Ks']), torch.from_numpy(z['poses']), device='cpu')
    key = lambda a: np.sort((a * 1e4).round().astype(np.int64).view([('', np.int64)] * 3), axis=0)
    assert np.array_equal(key(net.train_batch['rgbs'].numpy()), key(z['s1/rgbs']))
    assert not np.array_equal(net.train_batch['rgbs'].numpy(), z['s1/rgbs'])


@pytest.mark.parametrize('which,cfg', [('shape_bell', {}), ('shape_bear', {'shader_config': {'human_light': True}}),
                                       ('shape_sphdir', {'shader_config': {'sphere_direction': True}})])
def test_state_dict_surface_matches_reference_constructor(which, cfg):
    """keys, shapes and dtypes of the reference constructor's state_dict; a dict with that surface loads with strict=True"""
    man = json.load(open(os.path.join(GOLDEN, 'ref_state.json')))[which]
    net = _shape_net(cfg)
    sd = net.state_dict()
    assert set(sd.keys()) == set(man.keys())
    for k, (shape, dtype) in man.items():
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == dtype, k
    fake = {k: torch.full(shape, 0.25, dtype=getattr(torch, dtype.split('.')[1])) for k, (shape, dtype) in man.items()}
    net.load_state_dict(fake, strict=True)
    assert float(net.color_network.FG_LUT.mean()) == 0.25            # buffers are restored from the checkpoint too


@pytest.mark.parametrize('which,cfg', [('material_bell', {'human_lights': False, 'outer_light_version': 'direction'}),
                                       ('material_bear', {'human_lights': True, 'outer_light_version': 'sphere_direction'})])
def test_material_state_dict_surface(which, cfg):
    from tests.helpers import MatHolder
    man = json.load(open(os.path.join(GOLDEN, 'ref_state.json')))[which]
    net = MatHolder(cfg)
    sd = net.state_dict()
    assert set(sd.keys()) == set(man.keys())
    for k, (shape, dtype) in man.items():
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == dtype, k
    net.load_state_dict({k: torch.zeros(shape, dtype=getattr(torch, dtype.split('.')[1])) for k, (shape, dtype) in man.items()}, strict=True)


@pytest.mark.skipif(not os.path.exists('/root/reference/network/renderer.py'), reason='reference tree not present (GPU box)')
def test_reference_constructed_state_dict_loads_strict():
    """a state_dict produced by the REFERENCE constructor (through the import shim, in a subprocess: the shim patches torch and
    changes the working directory) loads into nero_amd with strict=True and yields identical effective weights"""
    code = (
        "import sys, torch; sys.path.insert(0, %r)\n"
        "from oracle import ref_shim\n"
        "renderer, field = ref_shim.load_reference()\n"
        "torch.manual_seed(11)\n"
        "ref = renderer.NeROShapeRenderer({'shader_config': {'human_light': True}}, training=False)\n"
        "sd = ref.state_dict()\n"
        "from nero_amd.renderer import NeROShapeRenderer\n"
        "torch.manual_seed(99)\n"
        "net = NeROShapeRenderer({'shader_config': {'human_light': True}}, training=False)\n"
        "r = net.load_state_dict(sd, strict=True)\n"
        "assert not r.missing_keys and not r.unexpected_keys\n"
        "W_ref = ref.sdf_network.lin3.weight if hasattr(ref.sdf_network.lin3, 'weight') else None\n"
        "W = net.sdf_network.effective()[3][0]\n"
        "g, v = sd['sdf_network.lin3.weight_g'], sd['sdf_network.lin3.weight_v']\n"
        "assert torch.allclose(W, g * v / v.norm(dim=1, keepdim=True), atol=1e-7)\n"
        "assert torch.equal(net.color_network.FG_LUT, sd['color_network.FG_LUT'])\n"
        "print('STRICT_OK', len(sd))\n" % ROOT)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert 'STRICT_OK 137' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_tracer_oracle_c_restatement_equals_numpy_oracle():
    from nero_amd.synthetic import icosphere
    from oracle.tracer_oracle import trace_bruteforce, trace_bruteforce_margins
    v, f = icosphere(3, 0.5, 0.15)
    f = np.ascontiguousarray(f[:, ::-1])
    rg = np.random.default_rng(0)
    o = rg.normal(size=(1500, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 2
    d = -o / 2 + rg.normal(size=(1500, 3)) * 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a = trace_bruteforce(v, f, o, d)
    b = trace_bruteforce_margins(v, f, o, d)
    assert np.array_equal(a[3], b[3]) and np.abs(a[2] - b[2]).max() < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12
    assert np.abs(a[0] - b[0]).max() < 1e-12
    assert 0.3 < (b[3] >= 0).mean() < 1.0 and b[4].mean() < 0.01


def test_secondary_ray_generator_for_the_tracer_tests():
    """nero_amd.synthetic.secondary_rays / camera_rays (inputs of tests/test_tracer.py and scripts/trace_bench.py): unit directions, point-major
    layout, origins 1e-3 off the surface on the outside, every direction in the outer half space of its triangle; against the brute-force
    oracle: a bumpy mesh is hit by some of them and a camera ray through the centre hits the front of the mesh"""
    from nero_amd.synthetic import camera_rays, icosphere, secondary_rays
    from oracle.tracer_oracle import trace_bruteforce
    v, f = icosphere(3, 0.5, 0.2)
    f = np.ascontiguousarray(f[:, ::-1])
    P, D = 40, 16
    o, d = secondary_rays(v, f, P, D, seed=3, device='cpu')
    assert o.shape == (P * D, 3) and d.shape == (P * D, 3) and o.dtype == torch.float32
    assert float((d.norm(dim=-1) - 1).abs().max()) < 1e-5
    ob = o.reshape(P, D, 3)
    assert float((ob - ob[:, :1]).abs().max()) == 0.0                         # the D rays of a point share its origin
    on, dn = o.numpy().astype(np.float64), d.numpy().astype(np.float64)
    # the origin is 1e-3 from the nearest triangle plane on its outer side: a ray straight back down hits at t = 1e-3
    tri = v[f].astype(np.float64)
    c = tri.mean(1)
    k = np.argmin(np.linalg.norm(c[None] - on[::D, None], axis=-1), axis=1)
    n = np.cross(tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where((n * c[k]).sum(1, keepdims=True) < 0, -n, n)
    assert np.abs(((on[::D] - c[k]) * n).sum(1) - 1e-3).max() < 1e-6
    assert ((dn.reshape(P, D, 3) * n[:, None]).sum(-1) > -1e-6).all()
    hit = trace_bruteforce(v, f, on, dn)[3] >= 0
    assert 0.02 < hit.mean() < 0.9
    co, cd = camera_rays(9, device='cpu')
    assert co.shape == (81, 3) and float((cd.norm(dim=-1) - 1).abs().max()) < 1e-6
    pos, nrm, depth, idx = trace_bruteforce(v, f, co.numpy().astype(np.float64), cd.numpy().astype(np.float64))
    assert idx[40] >= 0 and 1.0 < depth[40] < 2.0 and pos[40, 2] > 0               # the central ray: camera at z = 2, front of the mesh


def test_bench_gpus_flag_spawns_one_rank_per_gpu(monkeypatch):
    """`python bench.py --gpus N` without a torch.distributed environment re-launches itself under torch.distributed.run with
    N ranks on 127.0.0.1 (the flag used to be parsed and ignored)"""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    calls = {}
    monkeypatch.setattr(bench.torch.cuda, 'device_count', lambda: 8)
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd, env=None: calls.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '3', '--warmup', '1'])
    assert bench.spawn_ranks(8) == 0
    cmd = calls['cmd']
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1'] and '--nproc-per-node=8' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and cmd[-6:] == ['--gpus', '8', '--steps', '3', '--warmup', '1']
    assert calls['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'
    monkeypatch.setattr(bench.torch.cuda, 'device_count', lambda: 1)
    assert bench.spawn_ranks(2) == 2                                   # refuses to fake ranks it has no GPU for
    # the result line of a distributed run carries one record per rank (device, UUID, its own ms per step) and the backend that ran
    src = open(os.path.join(ROOT, 'bench.py')).read()
    for field in ("'rccl_ranks'", "'backend'", "'ranks'", "'uuid'", "'ms_per_step'", 'all_gather_object', "init_process_group('nccl')",
                  'FORCE_COLLECTIVES = True'):
        assert field in src, field


def test_forced_collectives_run_at_world_one_and_device_count_weights_match_the_host_version():
    """bench.py under torch.distributed.run with ONE rank sets parallel.FORCE_COLLECTIVES: the flat all-reduce and the count weights
    are then issued (gloo here) although world == 1 and must be the identity; device_count_weights equals global_count_weights"""
    import torch.distributed as dist
    from nero_amd import parallel
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(29650 + os.getpid() % 300))
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        p = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
        b = parallel.GradBucket(p)
        b.flat.copy_(torch.arange(b.flat.numel(), dtype=torch.float32))
        want = b.flat.clone()
        parallel.FORCE_COLLECTIVES = True
        b.all_reduce_mean(1)
        assert torch.equal(b.flat, want)
        w = parallel.device_count_weights([1234, 0], 1, 'cpu')
        assert w.dtype == torch.float32 and w.tolist() == [1.0, 1.0]
        # a count that lives on the device (the occlusion-loss candidates of the HIP-glued step, an int32 element) beside a host count
        w = parallel.device_count_weights([1234, torch.tensor([7, 99], dtype=torch.int32)[0]], 1, 'cpu')
        assert w.dtype == torch.float32 and w.tolist() == [1.0, 1.0] and parallel.parallel_forced()
        parallel.FORCE_COLLECTIVES = False
        assert parallel.device_count_weights([10, 3], 1, 'cpu').tolist() == parallel.global_count_weights([10, 3], 1, 'cpu')
    finally:
        parallel.FORCE_COLLECTIVES = False
        dist.destroy_process_group()


def test_workspace_sizes_hold_their_scratch_or_refuse():
    """Every *_workspace_bytes whose scratch is sized by asking hipCUB either reports a workspace that holds scratch beside its arrays, or
    refuses (0) and names itself and the failed query in nero_last_error() -- never a positive size with no scratch in it, which is what a size query whose status is thrown
    away yields on a machine without a device.  Launches nothing.  `arrays`: the 256-byte-aligned arrays and header of each documented layout."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib as L
    lib = L.bind(C.CDLL(os.path.join(ROOT, 'nero_amd', 'libnero_hip.so')))
    a = lambda nbytes: (nbytes + 255) // 256 * 256
    V, T, n, nt, px, grid = 1000, 2000, 1000, 2000, 8 * 8, 9 ** 3
    tiles = (grid + 2047) // 2048
    cases = [    # entry point, arguments, bytes of the arrays
        ('nero_mesh_compact_workspace_bytes', (V, T), 256 + 2 * a(4 * (V + 1)) + 2 * a(4 * (T + 1))),
        ('nero_mesh_cc_stats_workspace_bytes', (V, T), 3 * a(4 * (V + 1)) + 4 * a(4 * T) + a(8 * (T // 2048 + V + 1))),
        ('nero_mesh_chart_label_workspace_bytes', (T,), 2 * a(4 * (T + 1))),
        ('nero_mesh_chart_corners_workspace_bytes', (T,), 256 + 2 * a(8 * 3 * T) + 2 * a(4 * 3 * T) + 2 * a(4 * (3 * T + 1))),
        ('nero_voxel_downsample_workspace_bytes', (n,), 256 + a(1024 * 6 * 4) + a(8 * (n + 1)) + a(8 * n) + a(4 * (n + 1)) + a(4 * n)),
        ('nero_view_points_workspace_bytes', (8, 8), 2 * a(4 * (px + 1))),
        ('nero_uv_raster_workspace_bytes', (nt,), 256 + 2 * a(8 * (nt + 1))),
        ('nero_mcubes_workspace_bytes', (9, 9, 9), 256 + a(grid) + a(4 * grid) + 4 * a(8 * (tiles + 1))),
    ]
    assert cases[0][2] == 24832
    for name, args, arrays in cases:
        fn = getattr(lib, name)
        got = int(fn(*args))
        err = lib.nero_last_error()
        print(name, args, 'arrays', arrays, 'got', got, err)
        stem = name[:-len('_workspace_bytes')].encode()        # a message left by an earlier entry point does not count
        assert got > arrays or (got == 0 and stem in err and b'query' in err), (name, got, arrays, err)
