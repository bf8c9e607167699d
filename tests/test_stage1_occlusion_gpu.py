"""GPU tier: nero_stage1_occlusion (nero_amd/csrc/stage1_driver.hip) -- the occlusion-loss branch of the Stage-I step as one driver call on
a side stream -- against the launch sequence it replaces (nero_occ_candidates, nero_occ_select, nero_occ_gather and
nero_amd.shape_step.secondary_occlusion), bit for bit; the whole training step with and without side streams; the step workspace's size."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SN0, SN1 = 64, 16
_STATE = {}


def _step_state(R):
    """one training step at R rays (schedule step 25000): the driver keeps the forward state the occlusion branch reads.  Shared by the cases."""
    if R not in _STATE:
        from nero_amd.train import ShapeTrainStep
        ts = ShapeTrainStep({}, rays_per_rank=R, pool_rays=2 * R, device='cuda', variance=0.5, prime_fraction=0.0, prime_passes=0)
        c = ts.net.cfg
        g = torch.Generator().manual_seed(17 + R)
        rands = (torch.rand(R, 1, generator=g).cuda(), torch.rand(R, c['n_bg_samples'], generator=g).cuda(), torch.rand(R * ts.drv.T, generator=g).cuda())
        info = ts.forward_backward(25000, rands)
        torch.cuda.synchronize()
        assert ts._glue_obj is not None and info['n_in'] > 0
        d = ts.pool['d'][:R].contiguous()                    # the batch of that step (cursor 0)
        keys = torch.rand(R * ts.drv.T, generator=g).cuda()
        _STATE[R] = (ts, d, keys, info['n_in'])
    return _STATE[R]


def _reference(ts, d, keys, n_in, thresh, cap):
    """the Python-sequenced branch, as ShapeStepGlue.forward_backward issued it"""
    from nero_amd import _lib as L
    from nero_amd import stage1
    from nero_amd.chain import row_pad
    from nero_amd.shape_step import secondary_occlusion
    lib, p, drv = stage1._lib, stage1._p, ts.drv
    s = drv.state()
    assert s.n_in == n_in
    rpi = row_pad(n_in)
    x4, geo = drv._view(s.x4, (rpi, 4)), drv._view(s.geo, (rpi, 8))
    st = L.stream_ptr()
    flag = torch.empty(n_in, dtype=torch.uint8, device='cuda')
    cand = torch.full((cap,), -7, dtype=torch.int32, device='cuda')
    counts = torch.full((2,), -7, dtype=torch.int32, device='cuda')
    pts, dirs = torch.empty((cap, 3), device='cuda'), torch.empty((cap, 3), device='cuda')
    ws = torch.empty(lib.nero_occ_select_workspace(n_in), dtype=torch.uint8, device='cuda')
    L.check(lib.nero_occ_candidates(s.x4, s.sdf4, s.normal, s.inner_idx, p(d), drv.T, thresh, n_in, p(flag), st))
    L.check(lib.nero_occ_select(p(flag), n_in, p(keys), cap, p(cand), p(counts), ws.data_ptr(), ws.numel(), st))
    L.check(lib.nero_occ_gather(p(x4), p(geo), p(cand), cap, p(pts), p(dirs), st))
    var = ts.net.deviation_network.variance.detach()
    occ = secondary_occlusion(stage1._KAdapter(drv), pts, dirs, var, SN0, SN1)
    torch.cuda.synchronize()
    return cand, counts, occ


# (name, occ_sdf_thresh, cap, what the candidate total must be for the case to be the one it is meant to be)
CASES = [('fewer_than_cap', 0.01, 2048, lambda total, cap: 0 < total < cap),
         ('more_than_cap_7', 10.0, 7, lambda total, cap: total > cap),
         ('cap_1', 10.0, 1, lambda total, cap: total > cap),
         ('no_candidate', 0.0, 2048, lambda total, cap: total == 0)]


@pytest.mark.parametrize('side', [False, True], ids=['same_stream', 'side_stream'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('R', [64, 200])
def test_occlusion_entry_equals_the_python_sequence(R, case, side):
    """candidates, counts and the marched occlusion of nero_stage1_occlusion = those of the four calls it replaces, bit for bit, on the same
    driver state and the same keys; once with the branch on the caller's stream, once on a side stream"""
    from nero_amd import _lib as L
    from nero_amd import stage1
    lib, p = stage1._lib, stage1._p
    _, thresh, cap, expect = case
    ts, d, keys, n_in = _step_state(R)
    assert n_in % 64 != 0, n_in
    cand_r, counts_r, occ_r = _reference(ts, d, keys, n_in, thresh, cap)
    kept, total = counts_r.tolist()
    print(f'R {R} n_in {n_in} case {case[0]}: kept {kept} of {total} candidates, cap {cap}')
    assert expect(total, cap) and kept == min(total, cap), (kept, total, cap)
    var = ts.net.deviation_network.variance.detach()
    need = lib.nero_stage1_occlusion_workspace(ts.drv.h, n_in, cap, SN0, SN1)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    cand = torch.full((cap,), -9, dtype=torch.int32, device='cuda')
    counts = torch.full((2,), -9, dtype=torch.int32, device='cuda')
    occ = torch.full((cap,), -9.0, device='cuda')
    main = torch.cuda.current_stream()
    branch = main
    if side:
        branch = torch.cuda.Stream()
        branch.wait_stream(main)                              # (the buffers above were filled on the main stream)
    L.check(lib.nero_stage1_occlusion(ts.drv.h, p(d), p(var), p(keys), thresh, cap, SN0, SN1, p(cand), p(counts), p(occ), ws.data_ptr(), ws.numel(),
                                      branch.cuda_stream, main.cuda_stream))
    main.synchronize()                                        # the entry made the main stream wait for the branch: nothing else is needed
    assert counts.tolist() == [kept, total]
    assert torch.equal(cand, cand_r)
    assert torch.equal(occ.view(torch.int32), occ_r.view(torch.int32))
    # too small a scratch is refused in front of any launch
    assert lib.nero_stage1_occlusion(ts.drv.h, p(d), p(var), p(keys), thresh, cap, SN0, SN1, p(cand), p(counts), p(occ), ws.data_ptr(), 4096,
                                     branch.cuda_stream, main.cuda_stream) != 0
    torch.cuda.synchronize()


def _two_steps(monkeypatch, env):
    from nero_amd.train import ShapeTrainStep
    for k in ('NERO_STREAMS', 'NERO_MAT_FORK'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ts = ShapeTrainStep({}, rays_per_rank=256, pool_rays=1024, device='cuda', variance=0.5, prime_fraction=0.0, prime_passes=0)
    terms = []
    for i in range(2):
        info = ts.step(25000 + i)
        assert 'loss_terms' in info                            # the glued step: the one that calls nero_stage1_occlusion
        terms.append(info['loss_terms'].clone())
    torch.cuda.synchronize()
    params = torch.cat([q.detach().reshape(-1) for q in ts.net.parameters()]).clone()
    return torch.stack(terms), ts.bucket.flat.clone(), params


def test_two_training_steps_are_bit_identical_on_every_stream_setting(monkeypatch):
    """two optimisation steps at 256 rays, schedule step 25000: the default streams (occlusion branch on its side stream), NERO_STREAMS=1
    (everything on one stream) and NERO_MAT_FORK=1 (material predictors beside the normal pass) give the same loss terms, the same flat
    gradient bucket and the same parameters, bit for bit"""
    ref = _two_steps(monkeypatch, {})
    assert bool(torch.isfinite(ref[0]).all()) and float(ref[0][:, 3].abs().min()) > 0        # the occlusion term took part
    for env in ({'NERO_STREAMS': '1'}, {'NERO_MAT_FORK': '1'}, {'NERO_MAT_FORK': '0'}):
        got = _two_steps(monkeypatch, env)
        for name, a, b in zip(('loss_terms', 'gradient bucket', 'parameters'), ref, got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (env, name, float((a - b).abs().max()))


# nero_stage1_workspace_bytes_for(h, R, n_in, n_out, with_sampler = 1) of the library before the forward's launches were re-ordered, default
# streams, n_samples 64 + n_importance 64 + n_bg_samples 32, up_sample_steps 4: (human_light, sphere_direction, R, n_in, n_out) -> bytes
PARENT_BYTES = {(0, 0, 64, 5001, 3191): 1043362304, (0, 0, 256, 20000, 20960): 2704713472, (0, 0, 200, 0, 32000): 1262986752,
                (0, 0, 200, 32000, 0): 3242763264, (0, 0, 4096, 300000, 355360): 33807547392,
                (1, 1, 64, 5001, 3191): 1081969920, (1, 1, 256, 20000, 20960): 2857677824, (1, 1, 200, 0, 32000): 1262986752,
                (1, 1, 200, 32000, 0): 3487115264, (1, 1, 4096, 300000, 355360): 36098591744}


@pytest.mark.parametrize('mat_fork', ['0', '1'])
def test_step_workspace_size_is_unchanged(mat_fork, monkeypatch):
    from nero_amd import _lib as L
    from nero_amd import stage1
    lib = stage1._lib
    monkeypatch.delenv('NERO_STREAMS', raising=False)
    monkeypatch.setenv('NERO_MAT_FORK', mat_fork)
    for human, sphere in ((0, 0), (1, 1)):
        c = stage1.Cfg(64, 64, 32, 4, 1, human, sphere, 5.0, L.GEMM_F16X3, L.GEMM_F16X3, L.GEMM_F16X3, L.GEMM_F16X3)
        h = C.c_void_p()
        L.check(lib.nero_stage1_create(C.byref(c), C.byref(h)))
        try:
            for (hu, sp, R, n_in, n_out), want in PARENT_BYTES.items():
                if (hu, sp) == (human, sphere):
                    assert lib.nero_stage1_workspace_bytes_for(h, R, n_in, n_out, 1) == want, (human, sphere, R, n_in, n_out)
            # the occlusion branch's scratch query: positive inside the argument ranges, 0 outside, nothing launched either way
            assert lib.nero_stage1_occlusion_workspace(h, 5001, 2048, SN0, SN1) > 0
            assert lib.nero_stage1_occlusion_workspace(h, 0, 2048, SN0, SN1) == 0
            assert lib.nero_stage1_occlusion_workspace(h, 5001, 4097, SN0, SN1) == 0
        finally:
            lib.nero_stage1_destroy(h)
