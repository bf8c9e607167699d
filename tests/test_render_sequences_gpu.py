"""GPU tier: what happened BEFORE the call under test.  A renderer keeps a packed-kernel cache, its training pool's camera centres, a C
driver handle and a grow-only workspace across calls that differ in pose, ray count, chunk size and weights; every other GPU test
builds a fresh object per input.  Here call B after call A on one object must give what call B gives on a fresh object with the same
weights (tests.helpers.fresh_like), bit for bit: both are the same kernels on the same operands, and the library has fixed-order
reductions and no floating-point atomics (tests/test_determinism.py), so no tolerance is involved.  The one toleranced comparison is
the ray origin against the float64 camera centre (tests.helpers.centre_bound: 4 * 2^-24 * sum_j |R_ji| |t_j|), so that the sequences
do not rest on self-consistency alone.  Rule: DESIGN.md 9.14."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_bit_equal, centre_bound, fresh_like

pytestmark = pytest.mark.gpu

CFG = {'n_samples': 16, 'n_importance': 16, 'n_bg_samples': 8, 'apply_occ_loss': True, 'occ_loss_step': 20000, 'test_ray_num': 100,
       'test_downsample_ratio': False, 'train_ray_num': 128}
H, W = 20, 24                                              # 480 rays: four full chunks of 100 and a tail of 80
K = np.array([[45., 0, 12], [0, 45., 10], [0, 0, 1]], np.float32)
CAMS = ([0.5, -2.8, 0.6], [2.6, 0.9, 1.2], [-1.8, 2.0, -0.4], [-0.3, -1.2, 2.7], [2.0, -2.0, 0.9], [-2.9, -0.4, 0.5])


def _poses():
    from nero_amd.synthetic import look_at_pose
    return [look_at_pose(np.array(c, dtype=np.float64)) for c in CAMS]


def _shape_builder(**cfg):
    def build():
        from nero_amd.renderer import NeROShapeRenderer
        from nero_amd.synthetic import perturb_state
        torch.manual_seed(5)
        net = NeROShapeRenderer({**CFG, **cfg}, training=False)
        perturb_state(net, 0.4)                            # (a bumpy closed surface: the image is not flat)
        return net
    return build


def _spy_on_render(monkeypatch):
    """records (renderer, rays_o) of every NeROShapeRenderer.render call"""
    from nero_amd.renderer import NeROShapeRenderer
    seen, orig = [], NeROShapeRenderer.render

    def render(self, rays_o, *a, **k):
        seen.append((self, rays_o.detach().clone()))
        return orig(self, rays_o, *a, **k)
    monkeypatch.setattr(NeROShapeRenderer, 'render', render)
    return seen


def _assert_origins(rays_o, pose, where):
    c, bound = centre_bound(pose)
    err = np.abs(rays_o.cpu().numpy().astype(np.float64) - c[None])
    assert (err <= bound[None]).all(), (where, float((err / bound[None]).max()))


@pytest.mark.parametrize('extras', [False, True], ids=['c_inference_driver', 'python_sequenced_with_extras'])
def test_three_views_in_a_row_on_one_renderer(extras, monkeypatch):
    build = _shape_builder()
    net = build().cuda()
    A, B, C = _poses()[:3]
    seen = _spy_on_render(monkeypatch)
    outs = [net.render_image(p, K, H, W, extras=extras) for p in (A, B, C)]
    assert (getattr(net, '_infer_drv', None) is not None) == (not extras)
    if extras:
        assert {'depth', 'normal', 'occ_prob_gt', 'metallic', 'roughness'} <= set(outs[0])
    mine = [o for n, o in seen if n is net]
    assert len(mine) == 15 and [o.shape[0] for o in mine[5:10]] == [100, 100, 100, 100, 80]
    _assert_origins(torch.cat(mine[5:10]), B, 'view B after view A')
    _assert_origins(torch.cat(mine[10:]), C, 'view C after view B')
    assert float(outs[0]['ray_rgb'].std()) > 1e-3 and float((outs[0]['ray_rgb'] - outs[1]['ray_rgb']).abs().max()) > 1e-2
    for pose, got, name in ((B, outs[1], 'B'), (C, outs[2], 'C')):
        want = fresh_like(net, build).render_image(pose, K, H, W, extras=extras)
        assert_bit_equal(got, want, f'view {name} after the views before it')


def test_nvs_twice_on_one_renderer():
    build = _shape_builder()
    net = build().cuda()
    A, B = _poses()[:2]
    net.nvs(A, K, H, W)
    got = net.nvs(B, K, H, W)
    want = fresh_like(net, build).nvs(B, K, H, W)
    assert got.shape == (H, W, 3) and got.std() > 1e-3
    assert_bit_equal(got, want, 'nvs(B) after nvs(A)')


def test_test_step_over_two_views_and_back(monkeypatch):
    build = _shape_builder()
    net = build().cuda()
    A, B = _poses()[:2]
    info = {'imgs': torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(0)), 'Ks': torch.from_numpy(K).repeat(2, 1, 1),
            'poses': torch.from_numpy(np.stack([A, B]))}
    net.test_imgs_info, net.test_ids = info, [0, 1]
    seen = _spy_on_render(monkeypatch)
    r0 = net.test_step(0, 25000)
    r1 = net.test_step(1, 25000)
    r2 = net.test_step(0, 25000)
    mine = [o for n, o in seen if n is net]
    _assert_origins(torch.cat(mine[5:10]), B, 'test view 1 after test view 0')
    _assert_origins(torch.cat(mine[10:]), A, 'test view 0 after test view 1')
    assert r0['ray_rgb'].shape == (H, W, 3) and {'loss_rgb', 'gt_rgb', 'depth', 'normal'} <= set(r0)
    assert_bit_equal(r2, r0, 'test_step(0) after test_step(1)')
    fresh = fresh_like(net, build)
    fresh.test_imgs_info, fresh.test_ids = info, [0, 1]
    assert_bit_equal(r1, fresh.test_step(1, 25000), 'test_step(1) after test_step(0)')
    assert float((r1['ray_rgb'] - r0['ray_rgb']).abs().max()) > 1e-2


def test_train_validate_train_with_a_second_ray_pool(monkeypatch):
    """set_ray_pool(P1), a training step, a validation render, set_ray_pool(P2) -- same images and intrinsics, other poses; P1's tensors
    released in between, as a caller would -- and a training step: its ray_rgb is a fresh renderer's on P2 under the same seed (the
    shuffle, the sampler's perturbation and the occlusion keys all come from the device generator)"""
    build = _shape_builder()
    net = build().cuda()
    V = _poses()
    imgs = torch.rand(3, H, W, 3, generator=torch.Generator().manual_seed(1))
    Ks = torch.from_numpy(K).repeat(3, 1, 1)
    seen = _spy_on_render(monkeypatch)

    def pool_and_step(n, poses, seed):
        P = torch.from_numpy(np.stack(poses)).clone()
        torch.manual_seed(seed)
        n.set_ray_pool(imgs, Ks, P)
        del P
        idxs = n.train_batch['idxs'][:128].cpu().numpy()
        with torch.enable_grad():
            out = n.train_step(25000)
        assert getattr(n, '_train_drv', None) is not None                 # the drop-in step ran on the C driver
        return out['ray_rgb'].detach().clone(), out['loss_rgb'].detach().clone(), idxs

    pool_and_step(net, V[:3], 1)
    net.test_step(0, 25000)
    rgb, loss, idxs = pool_and_step(net, V[3:], 2)
    rays_o = [o for n, o in seen if n is net][-1]
    cb = [centre_bound(p) for p in V[3:]]
    err = np.abs(rays_o.cpu().numpy().astype(np.float64) - np.stack([cb[i][0] for i in idxs]))
    assert (err <= np.stack([cb[i][1] for i in idxs])).all(), 'the second pool is rendered from the first pool\'s cameras'
    rgb_f, loss_f, idxs_f = pool_and_step(fresh_like(net, build), V[3:], 2)
    assert np.array_equal(idxs, idxs_f)
    assert_bit_equal(rgb, rgb_f, 'ray_rgb of the step on the second pool')
    assert_bit_equal(loss, loss_f, 'loss_rgb of the step on the second pool')


def test_chunk_sizes_and_view_sizes_in_any_order_on_one_inference_driver():
    """one inference driver (packed once, one grow-only workspace): chunks of 100 (four full, a tail of 80), of 37, one chunk of 480 -- the
    same image; then a 7 x 5 view (35 rays, one partial block) behind the large ones -- a fresh renderer's; then the large view again"""
    build = _shape_builder()
    net = build().cuda()
    A, B = _poses()[:2]
    first = net.render_image(A, K, H, W, chunk=100)['ray_rgb']
    drv = net._infer_drv
    assert first.shape == (H * W, 3) and float(first.std()) > 1e-3
    for chunk in (37, 480):
        assert_bit_equal(net.render_image(A, K, H, W, chunk=chunk)['ray_rgb'], first, f'chunks of {chunk} after chunks of 100')
    Ks = np.array([[14., 0, 3.5], [0, 14., 2.5], [0, 0, 1]], np.float32)
    small = net.render_image(B, Ks, 5, 7)
    assert net._infer_drv is drv and small['ray_rgb'].shape == (35, 3)
    assert_bit_equal(small, fresh_like(net, build).render_image(B, Ks, 5, 7), '35 rays after 480')
    assert_bit_equal(net.render_image(A, K, H, W, chunk=100)['ray_rgb'], first, 'the large view again')
    assert net._infer_drv is drv


def test_material_renderer_views_in_a_row():
    from nero_amd.renderer import NeROMaterialRenderer
    from nero_amd.synthetic import icosphere, perturb_state
    v, f = icosphere(4, 0.5, 0.15)
    f = np.ascontiguousarray(f[:, ::-1])

    def build():
        torch.manual_seed(0)
        net = NeROMaterialRenderer({'shader_cfg': dict(diffuse_sample_num=32, specular_sample_num=16, human_lights=True,
                                                       outer_light_version='sphere_direction'),
                                    'database_name': 'real/x', 'test_ray_num': 100}, mesh=(v, f))
        perturb_state(net, None)
        return net
    net = build().cuda()
    A, B = _poses()[:2]
    info = {'imgs': torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(0)), 'Ks': torch.from_numpy(K).repeat(2, 1, 1),
            'poses': torch.from_numpy(np.stack([A, B]))}
    net.test_imgs_info = info
    verts = torch.from_numpy(v).cuda()
    m0 = net.predict_materials_of_vertices(verts)
    r0 = net.test_step(0)
    r1 = net.test_step(1)
    r2 = net.test_step(0)
    m1 = net.predict_materials_of_vertices(verts)
    hit = r0['rgb_gt'].abs().sum(-1) > 0
    assert 0.1 < float(hit.float().mean()) < 0.9 and float(r0['rgb_pr'][hit].std()) > 1e-4          # chunks with differing hit counts
    assert_bit_equal(r2, r0, 'test_step(0) after test_step(1)')
    fresh = fresh_like(net, build)
    fresh.test_imgs_info = info
    assert_bit_equal(r1, fresh.test_step(1), 'test_step(1) after test_step(0)')
    assert float((r1['rgb_pr'] - r0['rgb_pr']).abs().max()) > 1e-3
    assert_bit_equal(m1, m0, 'predict_materials_of_vertices after three test_steps')
    assert_bit_equal(m0, fresh.predict_materials_of_vertices(verts), 'predict_materials_of_vertices, fresh')


def test_ordered_trace_refuses_a_malformed_skip_mask_before_any_launch(monkeypatch):
    """RayTracer.trace_masked(chunk_order=...) -- the default Stage-II route -- reads n bytes at the mask's address: a mask of another
    type, size, device or layout is an AssertionError, and no entry point of the tracer is called"""
    from nero_amd import _lib as L
    from nero_amd.raytracing import RayTracer
    from nero_amd.synthetic import icosphere, secondary_rays
    v, f = icosphere(4, 0.5, 0.2)
    f = np.ascontiguousarray(f[:, ::-1])
    rt = RayTracer(v, f)
    order = [1, 0]
    o, d = secondary_rays(v, f, 10, 128, seed=2)
    o, d = o.cuda().contiguous(), d.cuda().contiguous()
    n = o.shape[0]
    skip = (torch.rand(n, generator=torch.Generator().manual_seed(1)) < 0.25).to(torch.uint8).cuda()
    want = [x.clone() for x in rt.trace_masked(o, d, skip)]
    calls = []
    for name in ('nero_bvh_trace_ordered', 'nero_bvh_trace_masked', 'nero_bvh_trace', 'nero_bvh_trace_grouped'):
        real = getattr(L.lib, name)
        monkeypatch.setattr(L.lib, name, lambda *a, _real=real, _name=name: calls.append(_name) or _real(*a))
    bad = {'int32': skip.to(torch.int32), 'one short': skip[:n - 1].contiguous(), 'on the host': skip.cpu(),
           'strided': torch.stack([skip, skip], 1)[:, 0]}
    assert not bad['strided'].is_contiguous() and bad['strided'].numel() == n
    for what, mask in bad.items():
        for kw in ({'chunk_order': order}, {}):                          # the ordered route and the plain masked one
            with pytest.raises(AssertionError):
                rt.trace_masked(o, d, mask, **kw)
    assert calls == []
    got = rt.trace_masked(o, d, skip, chunk_order=order)
    by_ptr = rt.trace_masked(o, d, skip.data_ptr(), chunk_order=order)   # an integer device pointer stays accepted
    assert calls == ['nero_bvh_trace_ordered'] * 2
    for a, b, c in zip(want, got, by_ptr):
        assert torch.equal(a, b) and torch.equal(a, c)
