"""GPU tier: one C driver handle across batch sizes, empty partitions and repacked weights.  Stage1Driver.workspace and
Stage2Driver.workspace grow and never shrink, and a handle holds the counts of its previous call: after a large batch a small one runs
with the large batch's rows lying behind its own in every workspace array.  tests/test_stage1_driver.py and test_stage2_driver.py run
one batch size per handle, over pad rows that a young process mostly finds zero.

Here every call on the reused handle must equal, bit for bit (torch.equal; tests.helpers.assert_bit_equal), the same call on a fresh
object with the same weights: a handle's result may depend only on its pack and its current arguments.  No poison is
written anywhere: the stale contents are the genuine larger call's, so whatever a kernel wrongly picks up was valid for that call and
lies inside the allocation -- a bug shows as a mismatch, not as a fault.  The one toleranced comparison is d loss / d variance, under
the rule tests/test_stage1_driver.py states for it (a 10^5-term sum): |a - b| <= 1e-5 |a| + 1e-12."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_bit_equal, fresh_like

pytestmark = pytest.mark.gpu

# ---- Stage I: the drop-in renderer's training route (NeROShapeRenderer._train_driver -> render -> loss -> backward) ------------------------
CFG1 = {'n_samples': 16, 'n_importance': 16, 'n_bg_samples': 8, 'freeze_inv_s_step': 15000, 'apply_occ_loss': True, 'occ_loss_step': 20000,
        'occ_loss_max_pn': 128}                                  # (a cap the large batches exceed and the small ones do not)
KINDS1 = {'bell': {}, 'bear': {'shader_config': {'human_light': True}}}
SIZES1 = (257, 33, 130, 3, 257)
STEP1 = 25000
_FRESH1 = {}                                                     # (kind, weights, R) -> the fresh object's result, computed once


def _builder1(kind):
    def build():
        from nero_amd.renderer import NeROShapeRenderer
        from nero_amd.synthetic import perturb_state
        torch.manual_seed(0)
        net = NeROShapeRenderer({**CFG1, **KINDS1[kind]}, training=False)
        perturb_state(net, 0.4)
        return net
    return build


def _inputs1():
    from nero_amd.synthetic import synthetic_rays
    o, d, poses, gt = synthetic_rays(max(SIZES1), seed=1, window=200)
    keys = torch.rand(max(SIZES1) * 40, generator=torch.Generator().manual_seed(9))       # one occlusion key per inner sample
    return [t.cuda() for t in (o, d, poses, gt, keys)]


def _step1(net, R, inputs):
    """forward + backward of R explicit rays through the renderer's own training driver, perturb_overwrite = 0, given occlusion keys"""
    from nero_amd.train import shape_training_loss
    o, d, poses, gt = (t[:R].contiguous() for t in inputs[:4])
    for p in net.parameters():
        p.grad = None
    near, far = net.near_far_from_sphere(o, d)
    kern, drv = net._train_driver(STEP1)
    assert drv is not None and drv is net._train_drv
    out = net.render(o, d, near, far, net.get_human_coordinate_poses(poses), 0, net.get_anneal_val(STEP1), is_train=True, step=STEP1,
                     occ_keys=inputs[4], _kern=kern, _driver=drv)
    loss = shape_training_loss(net, out, gt, STEP1)
    loss.backward()
    torch.cuda.synchronize()
    st = out['_state']
    return {'loss': loss.detach().clone(), 'n_in': st['n_in'], 'n_out': st['n_out'], 'occ_count': int(out.get('_occ_count', 0)),
            'ray_rgb': out['ray_rgb'].detach().clone(),
            'grads': {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}}


def _assert_same_step1(got, want, where):
    for k in ('loss', 'n_in', 'n_out', 'occ_count', 'ray_rgb'):
        assert_bit_equal(got[k], want[k], f'{where}: {k}')
    assert set(got['grads']) == set(want['grads'])
    for k, b in want['grads'].items():
        a = got['grads'][k]
        assert (a is None) == (b is None), (where, k)
        if b is None:
            continue
        if k == 'deviation_network.variance':              # the rule of tests/test_stage1_driver.py for this one scalar
            assert abs(float(a) - float(b)) <= 1e-5 * abs(float(a)) + 1e-12, (where, k, float(a), float(b))
        else:
            assert_bit_equal(a, b, f'{where}: d loss / d {k}')


def _fresh1(kind, net, R, inputs, weights='W1'):
    key = (kind, weights, R)
    if key not in _FRESH1:
        _FRESH1[key] = _step1(fresh_like(net, _builder1(kind)), R, inputs)
    return _FRESH1[key]


@pytest.mark.parametrize('streams', [None, '1'], ids=['default_streams', 'one_stream'])
@pytest.mark.parametrize('kind', list(KINDS1))
def test_stage1_handle_across_batch_sizes(kind, streams, monkeypatch):
    """R = 257, 33, 130, 3, 257 on one handle (the fresh handles run under the default NERO_STREAMS: the stream modes are bit-identical,
    tests/test_stage1_driver.py::test_stream_modes_are_bit_identical)"""
    inputs = _inputs1()
    net = _builder1(kind)().cuda()
    want = [_fresh1(kind, net, R, inputs) for R in SIZES1]
    if streams is not None:
        monkeypatch.setenv('NERO_STREAMS', streams)               # (read when the handle is created)
    drv, seen = None, []
    for i, R in enumerate(SIZES1):
        got = _step1(net, R, inputs)
        assert drv is None or net._train_drv is drv
        drv = net._train_drv
        _assert_same_step1(got, want[i], f'{kind}, call {i} at {R} rays after {SIZES1[:i]}')
        seen.append((got['n_in'], got['n_out'], got['occ_count']))
    assert all(n_in > 0 and n_out > 0 for n_in, n_out, _ in seen), seen
    assert seen[0][2] == CFG1['occ_loss_max_pn'] and 0 < seen[3][2] < CFG1['occ_loss_max_pn'], seen      # both sides of the cap
    assert float(max(g.abs().max() for g in want[3]['grads'].values() if g is not None)) > 0


@pytest.mark.parametrize('kind', list(KINDS1))
def test_stage1_repack_between_calls(kind):
    """pack W1, run; pack W2, run; pack W1, run -- on one handle, at two batch sizes: the third equals the first, the second a fresh
    handle packed with W2"""
    from nero_amd.synthetic import perturb_state
    inputs = _inputs1()
    build = _builder1(kind)
    net = build().cuda()
    w1 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    first = _step1(net, 130, inputs)
    drv = net._train_drv
    perturb_state(net, 0.45, seed=78)                             # W2, in place
    second = _step1(net, 33, inputs)
    other = fresh_like(net, build)
    _assert_same_step1(second, _step1(other, 33, inputs), 'W2 after W1')
    net.load_state_dict(w1, strict=True)
    third = _step1(net, 130, inputs)
    assert net._train_drv is drv
    _assert_same_step1(third, first, 'W1 again')
    _assert_same_step1(first, _fresh1(kind, net, 130, inputs), 'W1')
    assert float((first['ray_rgb'][:33] - second['ray_rgb']).abs().max()) > 1e-4


# ---- Stage II: MaterialTrainStep's route (C driver + HIP loss glue), one Stage2Driver ------------------------------------------------------
SCFGS = {'bear': dict(diffuse_sample_num=32, specular_sample_num=32, human_lights=True, outer_light_version='sphere_direction'),
         'bell_smith': dict(diffuse_sample_num=64, specular_sample_num=32, human_lights=False, outer_light_version='direction',
                            geometry_type='ggx_smith')}
SIZES2 = (130, 5, 65, 1, 130)
POOL2 = max(SIZES2)
_FRESH2 = {}


def _mesh2():
    from nero_amd.synthetic import icosphere
    v, f = icosphere(4, 0.5, 0.2)
    return v, np.ascontiguousarray(f[:, ::-1])


def _tracers2():
    """the mesh itself; the mesh out of reach (no secondary ray hits: the hit partition is empty); a closed shell of radius 4 around the
    points (every secondary ray hits: the miss partition is empty) -- the meshes of tests/test_edge_cases.py"""
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import icosphere
    v, f = _mesh2()
    vs, fs = icosphere(3, 4.0, 0.0)
    return {'none': RayTracer(v + np.array([[50.0, 0.0, 0.0]], dtype=v.dtype), f), 'shell': RayTracer(vs, np.ascontiguousarray(fs))}


def _new2(name, P):
    from nero_amd.train import MaterialTrainStep
    ts = MaterialTrainStep({'shader_cfg': SCFGS[name], 'database_name': 'real/bear'}, _mesh2(), points_per_rank=P, pool_points=POOL2,
                           device='cuda:0')
    assert ts.drv is not None and ts.fused_glue and ts.pool_n == POOL2
    return ts


def _rands2():
    g = torch.Generator().manual_seed(11)
    return {'rand_d': torch.rand(POOL2, 1, 1, generator=g).cuda(), 'rand_s': torch.rand(POOL2, 1, 1, generator=g).cuda(),
            'reg_ang': torch.rand(POOL2, 1, generator=g).cuda(), 'reg_eps': torch.normal(mean=0.0, std=0.05, size=[POOL2, 1], generator=g).cuda()}


def _step2(ts, P, rands, tracer=None):
    """forward + backward of the first P pool points on ts's handle; tracer: None (the renderer's own) or a RayTracer to shade against"""
    ts.P, ts.cursor = P, 0
    own = ts.net.ray_tracer
    if tracer is not None:
        ts.net.ray_tracer = tracer
    try:
        info = ts.forward_backward(5000, {k: v[:P].contiguous() for k, v in rands.items()})
    finally:
        ts.net.ray_tracer = own
    torch.cuda.synchronize()
    return {'loss': info['loss'].detach().clone(), 'loss_terms': info['loss_terms'].clone(), 'rgb_pr': info['out']['rgb_pr'].detach().clone(),
            'counts': tuple(ts.drv.last_counts), 'grads': ts.bucket.flat.clone()}


def _fresh2(name, P, rands, tracers, which=None, reweigh=None):
    key = (name, P, which, reweigh is not None)
    if key not in _FRESH2:
        ts = _new2(name, P)
        if reweigh is not None:
            reweigh(ts.net)
        _FRESH2[key] = _step2(ts, P, rands, tracers[which] if which else None)
    return _FRESH2[key]


@pytest.mark.parametrize('name', list(SCFGS))
def test_stage2_handle_across_batch_sizes(name):
    rands = _rands2()
    ts = _new2(name, SIZES2[0])
    drv = ts.drv
    for i, P in enumerate(SIZES2):
        got = _step2(ts, P, rands)
        assert ts.drv is drv and got['counts'][2] == P * (SCFGS[name]['diffuse_sample_num'] + SCFGS[name]['specular_sample_num'])
        assert_bit_equal(got, _fresh2(name, P, rands, None), f'{name}, call {i} at {P} points after {SIZES2[:i]}')
    n_miss, n_hit = got['counts'][:2]
    assert n_miss > 0 and n_hit > 0 and float(got['grads'].abs().max()) > 0


@pytest.mark.parametrize('name', list(SCFGS))
def test_stage2_empty_partitions_between_ordinary_batches(name):
    rands = _rands2()
    tracers = _tracers2()
    ts = _new2(name, 130)
    seq = [(130, None), (65, 'none'), (65, None), (65, 'shell'), (130, None)]
    for i, (P, which) in enumerate(seq):
        got = _step2(ts, P, rands, tracers[which] if which else None)
        n_miss, n_hit = got['counts'][:2]
        assert {None: n_miss > 0 and n_hit > 0, 'none': n_hit == 0 and n_miss > 0, 'shell': n_miss == 0 and n_hit > 0}[which], (which, got['counts'])
        assert_bit_equal(got, _fresh2(name, P, rands, tracers, which), f'{name}, call {i}: {P} points, mesh {which or "own"}, after {seq[:i]}')


@pytest.mark.parametrize('name', list(SCFGS))
def test_stage2_repack_between_calls(name):
    from nero_amd.synthetic import perturb_state
    rands = _rands2()
    ts = _new2(name, 130)
    w1 = {k: v.detach().clone() for k, v in ts.net.state_dict().items()}
    reweigh = lambda net: perturb_state(net, None, seed=78)
    first = _step2(ts, 130, rands)
    reweigh(ts.net)                                               # W2, in place: the next step repacks the same handle
    second = _step2(ts, 65, rands)
    assert_bit_equal(second, _fresh2(name, 65, rands, None, None, reweigh), 'W2 after W1')
    ts.net.load_state_dict(w1, strict=True)
    assert_bit_equal(_step2(ts, 130, rands), first, 'W1 again')
    assert_bit_equal(first, _fresh2(name, 130, rands, None), 'W1')
    assert float((first['rgb_pr'][:65] - second['rgb_pr']).abs().max()) > 1e-4
