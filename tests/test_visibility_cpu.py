"""CPU tier of the visibility queries (include/nero_hip_visibility.h; its binding: tests/test_binding_cpu.py): the entry points refuse
bad arguments before any device call, the numpy restatement of the AO sample set (tests/ao_ref.py) has the properties the kernels rely on,
ao_bytes is the rounded linear level, and the occlusion map travels through the OBJ / MTL writer and reader."""
import os

import numpy as np
import pytest
import torch

from tests import ao_ref as A
from tests.helpers import run_host_program

ERR_ARG = -1


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from nero_amd import _lib
    return _lib


def test_entry_points_refuse_bad_arguments_without_a_device(L):
    lib = L.lib
    p = 4096                                                          # a non-null pointer that is never followed: every call is refused first
    err = lambda: lib.nero_last_error().decode()
    # null handle / pointers
    for args in ((None, p, p, 4, None, 1.0, None, p, None), (p, None, p, 4, None, 1.0, None, p, None), (p, p, None, 4, None, 1.0, None, p, None),
                 (p, p, p, 4, None, 1.0, None, None, None), (None, p, p, 0, None, 1.0, None, p, None)):
        assert lib.nero_bvh_occluded(*args) == ERR_ARG and 'nero_bvh_occluded' in err()
    for bad in (0.0, -1.0, 10.5, float('nan'), float('inf')):
        assert lib.nero_bvh_occluded(p, p, p, 4, None, bad, None, p, None) == ERR_ARG and '(0, 10]' in err()
        assert lib.nero_bvh_occluded(p, p, p, 4, p, bad, None, p, None) == ERR_ARG   # with per-ray values too
        assert lib.nero_bvh_ao(p, p, p, p, 4, 8, 0, 0.0, bad, p, None) == ERR_ARG and '(0, 10]' in err()
    for k in range(5):
        a = [p, p, p, 4, 8, 0, 0.0, p, p, None]
        a[(0, 1, 2, 7, 8)[k]] = None
        assert lib.nero_ao_rays(*a) == ERR_ARG and 'nero_ao_rays' in err()
    for k in range(5):
        a = [p, p, p, p, 4, 8, 0, 0.0, 1.0, p, None]
        a[(0, 1, 2, 3, 9)[k]] = None
        assert lib.nero_bvh_ao(*a) == ERR_ARG and 'nero_bvh_ao' in err()
    for S in (0, 7, 12, 2048, -8):
        assert lib.nero_ao_rays(p, p, p, 4, S, 0, 0.0, p, p, None) == ERR_ARG and 'power of two' in err()
        assert lib.nero_bvh_ao(p, p, p, p, 4, S, 0, 0.0, 1.0, p, None) == ERR_ARG and 'power of two' in err()
    for n, S in ((A.MAX_RAYS // 8 + 1, 8), (1 << 21, 1024), ((1 << 31) - 1, 8)):
        assert n * S > A.MAX_RAYS
        assert lib.nero_ao_rays(p, p, p, n, S, 0, 0.0, p, p, None) == ERR_ARG and '2^31 - 64' in err()
        assert lib.nero_bvh_ao(p, p, p, p, n, S, 0, 0.0, 1.0, p, None) == ERR_ARG and '2^31 - 64' in err()
    assert lib.nero_ao_rays(p, p, p, -1, 8, 0, 0.0, p, p, None) == ERR_ARG
    # n = 0 with valid arguments: nothing to do, no device needed
    assert lib.nero_bvh_occluded(p, p, p, 0, None, 10.0, None, p, None) == 0
    assert lib.nero_ao_rays(p, p, p, 0, 64, 0, 0.0, p, p, None) == 0
    assert lib.nero_bvh_ao(p, p, p, p, 0, 64, 0, 0.0, 10.0, p, None) == 0


def test_grid_arithmetic_at_the_limit_under_the_sanitizer(tmp_path):
    """nero_amd/csrc/visibility_plan.h as a stand-alone program under the sanitizers (tests.helpers.run_host_program): at n * S = the largest
    admitted total, for every S and both workgroup sizes, the grid covers every ray, no index passes 2^31 - 1 and nothing overflows on the way"""
    rows = [tuple(int(x) for x in ln.split()) for ln in run_host_program(tmp_path, 'visibility_plan_main.cpp').splitlines()]
    assert len(rows) == 16
    for S, total, threads, blocks in rows:
        assert total == (A.MAX_RAYS // S) * S and total > A.MAX_RAYS - S
        assert blocks == -(-total // threads) and blocks * threads - 1 <= 2 ** 31 - 1
    assert (64, A.MAX_RAYS, 256, 1 << 23) in rows                     # total + 255 does not fit an int here


def _normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[0], v[1] = (0, 0, 1), (0, 0, -1)
    return v.astype(np.float32)


def test_the_sample_set_of_the_reference():
    nrm = _normals(32, 11)
    key = (np.arange(32) * 7919 + 5).astype(np.int32)
    for S in (8, 256):
        a, b = A.sample_ab(key, S, seed=3)
        assert a.shape == (32, S) and a.min() >= 0 and a.max() < 1 and b.min() >= 0 and b.max() < 1
        # one sample per stratum of a, whatever the rotation
        assert all(np.array_equal(np.sort(np.floor(a[j].astype(np.float64) * S).astype(int)), np.arange(S)) for j in range(32))
    o, d = A.ao_rays(np.zeros((32, 3), np.float32), nrm, key, 256, seed=3, bias=0.25)
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == (32 * 256, 3)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    cosn = (d.reshape(32, 256, 3).astype(np.float64) * nrm[:, None, :]).sum(-1)
    assert cosn.min() >= 0
    assert np.abs(cosn.mean(1) - 2 / 3).max() < 0.02                   # cosine weighting: E[cos] = 2/3
    assert np.array_equal(o.reshape(32, 256, 3)[:, 7], (0.25 * nrm.astype(np.float64)).astype(np.float32))
    t, u = A.frame(nrm)
    for x, y in ((t, u), (t, nrm), (u, nrm)):
        assert np.abs((x.astype(np.float64) * y).sum(-1)).max() < 1e-6
    assert np.abs(np.cross(t.astype(np.float64), u) - nrm).max() < 1e-6           # right-handed, at both poles too
    # another key or seed: another rotation of the same set
    o2, d2 = A.ao_rays(np.zeros((32, 3), np.float32), nrm, key + 1, 256, seed=3, bias=0.25)
    assert not np.array_equal(d, d2)
    assert int(A.lowbias32(0)) == 0 and len(set(A.lowbias32(np.arange(4096)).tolist())) == 4096     # 0 is fixed; the hash is a bijection


@pytest.mark.parametrize('S', [8, 64])
def test_ao_bytes_is_the_rounded_linear_level(S):
    from nero_amd.texture import ao_bytes
    c = np.arange(S + 1)
    got = ao_bytes(torch.from_numpy(c.astype(np.int32)), S)
    assert got.dtype == torch.uint8
    got = got.numpy()
    assert got[0] == 255 and got[S] == 0 and np.all(np.diff(got.astype(int)) < 0)
    assert np.array_equal(got, np.floor(255.0 * (S - c) / S + 0.5).astype(np.uint8))
    assert np.array_equal(got, A.ao_bytes(c, S))


def test_the_occlusion_map_round_trips_through_the_obj(tmp_path):
    from nero_amd import texture as TX
    rng = np.random.default_rng(4)
    v = rng.normal(size=(5, 3))
    f = np.array([[0, 1, 2], [2, 3, 4]])
    vt, ft = TX.simple_atlas(v, f, 16)
    maps = {'albedo': rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), 'metallic': rng.integers(0, 256, (16, 16), dtype=np.uint8),
            'roughness': rng.integers(0, 256, (16, 16), dtype=np.uint8)}
    plain = tmp_path / 'plain'
    obj = TX.write_textured_obj(str(plain), v, f, vt, ft, maps, use_pil=False)
    assert sorted(os.listdir(plain)) == ['feat0_0.png', 'feat1_0.png', 'feat2_0.png', 'mesh_0.mtl', 'mesh_0.obj']
    assert 'map_Ka' not in open(plain / 'mesh_0.mtl').read()
    back = TX.read_textured_obj(obj)
    assert 'ao' not in back and 'map_Ka' not in back
    with_ao = tmp_path / 'ao'
    ao = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    obj2 = TX.write_textured_obj(str(with_ao), v, f, vt, ft, {**maps, 'ao': torch.from_numpy(ao)}, use_pil=False)
    assert sorted(os.listdir(with_ao)) == ['feat0_0.png', 'feat1_0.png', 'feat2_0.png', 'feat3_0.png', 'mesh_0.mtl', 'mesh_0.obj']
    mtl = open(with_ao / 'mesh_0.mtl').read()
    assert mtl == open(plain / 'mesh_0.mtl').read() + 'map_Ka feat3_0.png\n'
    for name in ('feat0_0.png', 'feat1_0.png', 'feat2_0.png', 'mesh_0.obj'):      # the other files are what they are without 'ao'
        assert open(with_ao / name, 'rb').read() == open(plain / name, 'rb').read()
    back = TX.read_textured_obj(obj2)
    assert back['map_Ka'] == 'feat3_0.png' and np.array_equal(back['ao'], ao)
    for k in ('albedo', 'metallic', 'roughness'):
        assert np.array_equal(back[k], maps[k])
