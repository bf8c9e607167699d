"""Plain torch / numpy restatement of the Stage-I step glue (nero_amd/csrc/step_glue.hip): one function per entry point, dtype-generic
(one source serves float64 and float32), evaluated on the kernel's own float32 inputs; backward references are float64 autograd of the
forwards, so every tie is torch's (sign(0) = 0, smooth-L1 takes x / beta at |x| == beta, clip passes the gradient on its bounds).  Also the
case tables, the input generators and the judging rule that tests/test_step_glue_kernels_gpu.py (the kernels) and
tests/test_glue_ref_cpu.py (this file) share.  No GPU is touched here.

Judging rule.  Integers, copies, zeros, refusals and guards are exact.  Element-wise float outputs: per row, |got - ref64| / max(|ref64| of
the row, unit of the row) <= max(3 x floor, 8 x 2^-24), the floor being the worst row of the float32 restatement against the float64 one
over ALL cases of the entry point's family (computed on the CPU).  A loss term is a mean of N non-negative float32 terms summed in the
fixed order of the kernels -- a 256-wide tree per block (8 levels), a strided pass over the nb = ceil(N / 256) block partials
(ceil(nb / 256) additions per thread), a 256-wide tree (8 levels) -- so its relative distance from the float64 value is at most
(16 + ceil(nb / 256) + 6) x 2^-24, six roundings being allowed for forming one term and for the final scale; the total gets two more.
That bound is derived, not measured; no bound here is computed from a kernel's output."""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24
FLOOR_FACTOR, ROUNDINGS = 3.0, 8
TINY = 1e-300                                      # keeps 0 / 0 of an all-zero reference row from being NaN: the kernel must give exact zeros there
LB, SB, PICK_MAX = 256, 1024, 4096                 # step_glue.hip: threads per block, samples per scan block, the largest cap
NEAR_MIN = float(np.float32(1e-3))                 # the clamp of near: the kernel's (and ATen's) float32 constant
KINDS = ('l2', 'l1', 'smooth_l1', 'charbonier')    # index = NERO_RGB_*
EIK_W = float(np.float32(0.1))                     # eik_weight travels through the C ABI as a float
WEIGHTS = (None, (float(np.float32(0.7)), float(np.float32(1.9))))
D_LOSS = float(np.float32(0.7))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


# ---- the judging rule ----------------------------------------------------------------------------------------------------------------
def row_err(a, ref, unit=0.0):
    """worst row of |a - ref| / max(|ref| of the row, unit of the row); an element of a 1-D output is its own row"""
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not a.numel():
        return 0.0
    a, ref = a.double().reshape(a.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    rows = ref.abs().max(-1)[0].clamp(min=TINY)
    if torch.is_tensor(unit):
        rows = torch.maximum(rows, unit.double().reshape(a.shape[0], -1).max(-1)[0])
    else:
        rows = rows.clamp(min=max(unit, TINY))
    return ((a - ref).abs().max(-1)[0] / rows).max().item()


def bound_of(floor):
    return max(FLOOR_FACTOR * floor, ROUNDINGS * EPS32)


def scan_rounds(n):
    """iterations of occ_scan_kernel's loop: one per 256 scan blocks of 1024 samples"""
    return -(-(-(-n // SB)) // LB)


def loss_rounds(N):
    """additions per thread of loss_final_kernel's strided pass over the block partials of N terms"""
    return -(-(-(-N // LB)) // LB)


def loss_bound(N, extra=0):
    """relative bound of a mean of N non-negative float32 terms summed in the kernels' fixed order (module docstring)"""
    return (22 + max(1, loss_rounds(N)) + extra) * EPS32


def rel(a, ref):
    a, ref = float(a), float(ref)
    return 0.0 if a == ref else abs(a - ref) / max(abs(ref), TINY)


# ---- nero_near_far_sphere -------------------------------------------------------------------------------------------------------------
NEAR_FAR_R = (1, 255, 256, 257, 1000)
RAY_KINDS = ('unit', 'dir_x1e-3', 'dir_x1e3', 'origin_1e-3', 'origin_on_sphere', 'origin_1e3', 'through_centre', 'perpendicular', 'inside_half')
INSIDE = (RAY_KINDS.index('origin_1e-3'), RAY_KINDS.index('inside_half'))


@functools.lru_cache(maxsize=None)
def near_far_inputs(R, shift=0):
    """float32 rays, ray i of kind RAY_KINDS[(i + shift) % 9]: unit directions towards a point of the unit ball from distance 3; the same
    with the direction scaled by 1e-3 / 1e3; origins at distance 1e-3 (inside), 1 and 1e3; rays through the centre; rays nearly
    perpendicular to o (o.d cancels); origins at distance 0.5 (inside)"""
    g = _gen('near_far', R, shift)
    kind = (torch.arange(R) + shift) % len(RAY_KINDS)
    u = F.normalize(torch.randn(R, 3, generator=g, dtype=F64), dim=-1)
    target = F.normalize(torch.randn(R, 3, generator=g, dtype=F64), dim=-1) * torch.rand(R, 1, generator=g, dtype=F64) ** (1 / 3) * 0.9
    dist = torch.full((R, 1), 3.0, dtype=F64)
    for name, v in (('origin_1e-3', 1e-3), ('origin_on_sphere', 1.0), ('origin_1e3', 1e3), ('inside_half', 0.5)):
        dist[kind == RAY_KINDS.index(name)] = v
    o = u * dist
    d = F.normalize(target - o, dim=-1)
    k = kind == RAY_KINDS.index('through_centre')
    d[k] = -u[k]
    k = kind == RAY_KINDS.index('perpendicular')
    side = F.normalize(torch.cross(u, torch.randn(R, 3, generator=g, dtype=F64), dim=-1), dim=-1)
    d[k] = F.normalize(side - 1e-4 * u, dim=-1)[k]
    d[kind == RAY_KINDS.index('dir_x1e-3')] *= 1e-3
    d[kind == RAY_KINDS.index('dir_x1e3')] *= 1e3
    return dict(o=o.float().contiguous(), d=d.float().contiguous(), kind=kind)


def near_far(o, d, dtype=F64):
    """network/renderer.py:231-238 -> near [R], far [R], unit [R] (float64): mid is a quotient of a three-term dot product that can cancel
    and near = mid - 1 a difference from 1, so a row is measured against max(|value|, 1, sum_c |o_c d_c| / d.d)"""
    unit = ((o.double() * d.double()).abs().sum(-1) / (d.double() ** 2).sum(-1)).clamp(min=1.0)
    o, d = o.to(dtype), d.to(dtype)
    a = torch.sum(d ** 2, dim=-1)
    b = 2.0 * torch.sum(o * d, dim=-1)
    mid = 0.5 * (-b) / a
    return torch.clamp(mid - 1.0, min=NEAR_MIN), mid + 1.0, unit


def near_far_family():
    """every input set of the family: (R, shift)"""
    return [(R, 0) for R in NEAR_FAR_R if R > 1] + [(1, s) for s in range(len(RAY_KINDS))]


@functools.lru_cache(maxsize=None)
def near_far_floors():
    out = {'near': 0.0, 'far': 0.0}
    for R, s in near_far_family():
        q = near_far_inputs(R, s)
        n64, f64, unit = near_far(q['o'], q['d'])
        n32, f32, _ = near_far(q['o'], q['d'], F32)
        out['near'], out['far'] = max(out['near'], row_err(n32, n64, unit)), max(out['far'], row_err(f32, f64, unit))
    return out


# ---- nero_occ_select ------------------------------------------------------------------------------------------------------------------
def occ_select(flag, keys, cap):
    """the contract of include/nero_hip.h: counts = (kept, total); cand [cap] = the sample indices of the kept candidates in ascending
    order, -1 in the unused slots; kept = argsort(keys[:total], stable)[:cap] over the candidates' ordinals.  numpy's stable argsort puts
    +inf behind every finite key and NaN behind +inf, ties to the lower ordinal."""
    every = np.nonzero(np.asarray(flag))[0]
    total = int(every.size)
    order = np.argsort(np.asarray(keys, np.float32)[:total], kind='stable')[:cap]
    kept = np.sort(every[order])
    cand = np.full(cap, -1, np.int32)
    cand[:kept.size] = kept
    return cand, (int(kept.size), total)


def occ_select_inf_for_the_rest(flag, keys, cap):
    """NOT the contract: the rule of a sort that gives every non-candidate the float key +inf (one stable sort over all n samples by
    (key or +inf, sample index), the first min(total, cap) records, sorted).  tests/test_glue_ref_cpu.py uses it to show that the +inf
    cases can tell the two rules apart."""
    flag = np.asarray(flag) != 0
    n, total = flag.size, int(flag.sum())
    skey = np.full(n, np.inf, np.float32)
    skey[flag] = np.asarray(keys, np.float32)[:total]
    kept = np.sort(np.argsort(skey, kind='stable')[:min(total, cap)])
    cand = np.full(cap, -1, np.int32)
    cand[:kept.size] = kept
    return cand, (int(kept.size), total)


# name -> (n, cap, candidate layout, key set, total against cap, scan blocks against 256)
#   layout: none | all | first | last | last_block | from:I:p (each sample >= I with probability p) | frac:p | exact (total == cap) |
#           plus1 (total == cap + 1) | bytes:p (as frac, the set flag bytes being 1, 2 or 255) | bits:0101... (literally)
#   keys:   random | ties16 | equal | inf_tail:F (finite for the ordinals < F, +inf behind: how both callers pad) | inf_head:F (finite only
#           for the LAST F candidates) | nan_tail:F:I (F finite ordinals, then I of +inf, then NaN) | signed_zeros (-0.0, +0.0 and 0.25)
#   total:  zero | below | equal | plus1 | above the cap;   blocks: ceil(n / 1024) <, == or > 256
SELECT_CASES = {
    'n1_all_cap1': (1, 1, 'all', 'random', 'equal', '<'),
    'n1_none_cap3': (1, 3, 'none', 'random', 'zero', '<'),
    'n1_all_cap4096': (1, 4096, 'all', 'equal', 'below', '<'),
    'n1023_half_cap100': (1023, 100, 'frac:0.5', 'random', 'above', '<'),
    'n1024_all_cap4095_ties': (1024, 4095, 'all', 'ties16', 'below', '<'),
    'n1024_total_is_cap100': (1024, 100, 'exact', 'random', 'equal', '<'),
    'n1025_total_is_cap100_plus1': (1025, 100, 'plus1', 'random', 'plus1', '<'),
    'n1025_only_last_cap2': (1025, 2, 'last', 'random', 'below', '<'),
    'n1025_only_first_cap1': (1025, 1, 'first', 'random', 'equal', '<'),
    'n1025_total_is_cap2_plus1': (1025, 2, 'plus1', 'ties16', 'plus1', '<'),
    'n4097_all_cap4096': (4097, 4096, 'all', 'random', 'plus1', '<'),
    'n4097_all_cap4095_ties': (4097, 4095, 'all', 'ties16', 'above', '<'),
    'n4097_equal_keys_cap3': (4097, 3, 'frac:0.3', 'equal', 'above', '<'),
    'n4097_flag_bytes_cap100': (4097, 100, 'bytes:0.4', 'random', 'above', '<'),
    'n4097_total_is_cap4095': (4097, 4095, 'exact', 'random', 'equal', '<'),
    'n262144_last_block_cap100': (262144, 100, 'last_block', 'random', 'above', '=='),
    'n262144_third_cap4096': (262144, 4096, 'frac:0.3', 'random', 'above', '=='),
    'n262144_all_cap4096_ties': (262144, 4096, 'all', 'ties16', 'above', '=='),
    'n262145_third_cap4095': (262145, 4095, 'frac:0.3', 'random', 'above', '>'),
    'n262145_only_last_cap1': (262145, 1, 'last', 'random', 'equal', '>'),
    'n262145_total_is_cap4096': (262145, 4096, 'exact', 'random', 'equal', '>'),
    'n263169_third_cap4096_ties': (263169, 4096, 'frac:0.3', 'ties16', 'above', '>'),
    'n263169_total_is_cap100_plus1': (263169, 100, 'plus1', 'random', 'plus1', '>'),
    'n263169_flag_bytes_cap3': (263169, 3, 'bytes:0.5', 'equal', 'above', '>'),
    'n263169_none_cap100': (263169, 100, 'none', 'random', 'zero', '>'),
    'n263169_all_cap4096': (263169, 4096, 'all', 'random', 'above', '>'),
    'n263169_only_last_cap2': (263169, 2, 'last', 'random', 'below', '>'),
    'n263169_second_round_blocks_cap100': (263169, 100, 'from:262144:0.5', 'random', 'above', '>'),
    'inf_issue_example_cap4': (12, 4, 'bits:010110010101', 'inf_tail:2', 'above', '<'),
    'inf_total_below_cap100': (1025, 100, 'frac:0.05', 'inf_tail:10', 'below', '<'),
    'inf_all_keys_cap3': (1023, 3, 'frac:0.5', 'inf_tail:0', 'above', '<'),
    'inf_fewer_finite_than_cap100': (4097, 100, 'frac:0.4', 'inf_tail:30', 'above', '<'),
    'inf_more_finite_than_cap100': (4097, 100, 'frac:0.4', 'inf_tail:300', 'above', '<'),
    'inf_finite_keys_on_the_last_candidates_cap100': (4097, 100, 'frac:0.4', 'inf_head:20', 'above', '<'),
    'inf_fewer_finite_than_cap4096_two_rounds': (263169, 4096, 'frac:0.3', 'inf_tail:1000', 'above', '>'),
    'inf_then_nan_keys_cap100': (4097, 100, 'frac:0.4', 'nan_tail:30:20', 'above', '<'),
    'signed_zero_keys_cap100': (4097, 100, 'frac:0.4', 'signed_zeros', 'above', '<'),
}
# the +inf cases in which fewer candidates hold a finite key than are kept: the kept set then reaches into the +inf keys
INF_SHORT = ('inf_issue_example_cap4', 'inf_total_below_cap100', 'inf_all_keys_cap3', 'inf_fewer_finite_than_cap100',
             'inf_finite_keys_on_the_last_candidates_cap100', 'inf_fewer_finite_than_cap4096_two_rounds', 'inf_then_nan_keys_cap100')
INF_LONG = ('inf_more_finite_than_cap100',)       # more finite keys than the cap: no +inf key is kept


@functools.lru_cache(maxsize=None)
def select_inputs(name):
    """-> flag uint8 [n], keys float32 [n] (numpy; the kernel reads keys[ordinal], ordinal < total <= n)"""
    n, cap, layout, kset = SELECT_CASES[name][:4]
    r = _rng('select', name)
    flag = np.zeros(n, np.uint8)
    kind, _, arg = layout.partition(':')
    if kind == 'all':
        flag[:] = 1
    elif kind == 'first':
        flag[0] = 1
    elif kind == 'last':
        flag[n - 1] = 1
    elif kind == 'last_block':
        lo = (n - 1) // SB * SB
        flag[lo:] = r.random(n - lo) < 0.5
    elif kind == 'from':
        lo, p = int(arg.split(':')[0]), float(arg.split(':')[1])
        flag[lo:] = r.random(n - lo) < p
        flag[n - 1] = 1
    elif kind == 'frac':
        flag[:] = r.random(n) < float(arg)
    elif kind in ('exact', 'plus1'):
        flag[r.permutation(n)[:cap + (kind == 'plus1')]] = 1
    elif kind == 'bytes':
        flag[:] = np.where(r.random(n) < float(arg), r.choice(np.array([1, 2, 255], np.uint8), n), 0)
    elif kind == 'bits':
        flag[:] = [int(c) for c in arg]
    else:
        assert kind == 'none', layout
    total = int(np.count_nonzero(flag))
    keys = r.random(n, dtype=np.float32)
    kind, _, arg = kset.partition(':')
    if kind == 'ties16':
        keys = np.floor(keys * 16) / 16
    elif kind == 'equal':
        keys[:] = 0.5
    elif kind == 'inf_tail':
        keys[int(arg):] = np.inf
    elif kind == 'inf_head':
        keys[:total - int(arg)] = np.inf
        keys[total:] = np.inf
    elif kind == 'nan_tail':
        fin, ninf = (int(x) for x in arg.split(':'))
        keys[fin:fin + ninf] = np.inf
        keys[fin + ninf:] = np.nan
    elif kind == 'signed_zeros':
        keys = r.choice(np.array([-0.0, 0.0, 0.25], np.float32), n)
    else:
        assert kind == 'random', kset
    return flag, keys.astype(np.float32)


# ---- nero_occ_gather -------------------------------------------------------------------------------------------------------------------
GATHER_CASES = [(1, 'full'), (1, 'holes'), (255, 'holes'), (256, 'holes'), (256, 'full'), (257, 'holes')]


@functools.lru_cache(maxsize=None)
def gather_inputs(cap, variant):
    """x4 [n,4], geo [n,8]: every element a different number (row and column readable from it), cand [cap] ascending with -1 slots at the
    end and -- 'holes' -- scattered in the middle"""
    n = 3 * cap + 7
    x4 = (torch.arange(n * 4, dtype=F32) + 0.5).reshape(n, 4)
    geo = -(torch.arange(n * 8, dtype=F32) + 0.25).reshape(n, 8)
    cand = torch.sort(torch.randperm(n, generator=_gen('gather', cap, variant))[:cap])[0].int()
    if variant == 'holes':
        cand[torch.arange(cap) % 5 == 2] = -1
        cand[cap - cap // 4 - 1:] = -1
    return dict(x4=x4, geo=geo, cand=cand)


def occ_gather(x4, geo, cand):
    """pts / dirs [cap,3] = x4[cand, 0:3] / geo[cand, 4:7]; unused slots: the origin and +z"""
    used = (cand >= 0)[:, None]
    i = cand.clamp(min=0).long()
    pts = torch.where(used, x4[i, :3], torch.zeros(1, 3, dtype=x4.dtype))
    dirs = torch.where(used, geo[i, 4:7], torch.tensor([[0.0, 0.0, 1.0]], dtype=geo.dtype))
    return pts, dirs


# ---- nero_occ_l1 / nero_occ_l1_backward -----------------------------------------------------------------------------------------------
# (cap, kept, n_in): cap = 1, 1023, 1024, 1025, 4096 (the 1024-thread block and its stride); kept = cap, cap // 3, 1, 0; n_in = 1, 4097, 70001
L1_CASES = [(1, 1, 1), (1, 0, 1), (1, 1, 4097), (1023, 1023, 4097), (1023, 341, 70001), (1023, 1, 1), (1024, 1024, 4097), (1024, 341, 4097),
            (1024, 0, 70001), (1025, 1025, 70001), (1025, 341, 4097), (1025, 1, 4097), (4096, 4096, 4097), (4096, 1365, 70001), (4096, 1, 1),
            (4096, 0, 4097)]


@functools.lru_cache(maxsize=None)
def l1_inputs(cap, kept, n_in):
    """occ [n_in], cand [cap] (kept ascending samples, then -1), counts (kept, total) -- (0, 0) without a candidate --, gt [cap] with one exact
    tie occ == gt at slot kept // 2 once kept >= 2"""
    g = _gen('occ_l1', cap, kept, n_in)
    occ = torch.rand(n_in, generator=g)
    cand = torch.full((cap,), -1, dtype=torch.int32)
    cand[:kept] = torch.sort(torch.randperm(n_in, generator=g)[:kept])[0].int()
    gt = torch.rand(cap, generator=g)
    if kept >= 2:
        gt[kept // 2] = occ[cand[kept // 2].long()]
    counts = torch.tensor([kept, kept + 5 if kept else 0], dtype=torch.int32)
    return dict(occ=occ, cand=cand, counts=counts, gt=gt)


def occ_l1(occ, cand, counts, gt):
    """sum over the used slots k of |occ[cand[k]] - gt[k]| / max(counts[0], 1); in the dtype of occ"""
    used = cand >= 0
    return ((occ[cand.clamp(min=0).long()] - gt.to(occ.dtype)).abs() * used).sum() / max(int(counts[0]), 1)


def occ_l1_fwd_bwd(q, dtype=F64):
    """-> loss, d_occ [n_in] = D_LOSS * d loss / d occ by autograd"""
    a = leaf(q['occ'], dtype)
    loss = occ_l1(a, q['cand'], q['counts'], q['gt'])
    g, = torch.autograd.grad(loss * D_LOSS, a)
    return loss.detach(), g


@functools.lru_cache(maxsize=None)
def l1_floor():
    return max(row_err(occ_l1_fwd_bwd(l1_inputs(*c), F32)[1], occ_l1_fwd_bwd(l1_inputs(*c))[1]) for c in L1_CASES)


# ---- nero_shape_loss --------------------------------------------------------------------------------------------------------------------
# (R, n_in): one row; across the 256-thread blocks on either side; more than 256 blocks on the sample side and on the ray side (258 each: a
# second strided round of loss_final_kernel); exactly 257 blocks (only thread 0 takes a second partial)
LOSS_SHAPES = [(1, 0), (1, 1), (255, 257), (257, 255), (256, 256), (700, 65793), (66000, 300), (300, 65537)]
LOSS_CAP = 300
OCC_MODES = ('none', 'kept0', 'kept1', 'full')     # cand = NULL; cand present with 0, 1 and cap = 300 kept candidates


def occ_modes(n_in):
    return [m for m in OCC_MODES if m == 'none' or (n_in > 0 and (m != 'full' or n_in >= LOSS_CAP))]


def loss_family():
    return [(R, n_in, m) for R, n_in in LOSS_SHAPES for m in occ_modes(n_in)]


@functools.lru_cache(maxsize=None)
def loss_inputs(R, n_in, mode):
    """rgb / gt [R,3] with (R >= 3) row 0 rgb == gt exactly and rows 1, 2 at |rgb - gt| == 0.25 exactly in both signs (the smooth-L1 joint:
    multiples of 1 / 256, so the float32 difference is exact); gerr, occ [n_in]; the occlusion arguments of `mode`, with one tie
    occ == gt_occ when 300 candidates are kept"""
    g = _gen('shape_loss', R, n_in, mode)
    rgb, gt = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    if R >= 3:
        rgb[0] = gt[0]
        gt[1:3] = torch.randint(64, 193, (2, 3), generator=g).float() / 256
        rgb[1] = gt[1] + torch.tensor([0.25, -0.25, 0.25])
        rgb[2] = gt[2] + torch.tensor([-0.25, 0.25, -0.25])
    q = dict(rgb=rgb, gt=gt, gerr=torch.rand(n_in, generator=g), occ=torch.rand(n_in, generator=g), cand=None, counts=None, gt_occ=None)
    if mode != 'none':
        kept = {'kept0': 0, 'kept1': 1, 'full': LOSS_CAP}[mode]
        q['cand'] = torch.full((LOSS_CAP,), -1, dtype=torch.int32)
        q['cand'][:kept] = torch.sort(torch.randperm(n_in, generator=g)[:kept])[0].int()
        q['counts'] = torch.tensor([kept, 4 * kept], dtype=torch.int32)
        q['gt_occ'] = torch.rand(LOSS_CAP, generator=g)
        if kept >= 2:
            q['gt_occ'][kept // 2] = q['occ'][q['cand'][kept // 2].long()]
    return q


def rgb_loss(kind, rgb_pr, rgb_gt):
    """network/renderer.py:332-343, per ray"""
    if KINDS[kind] == 'l2':
        return torch.sum((rgb_pr - rgb_gt) ** 2, -1)
    if KINDS[kind] == 'l1':
        return torch.sum(F.l1_loss(rgb_pr, rgb_gt, reduction='none'), -1)
    if KINDS[kind] == 'smooth_l1':
        return torch.sum(F.smooth_l1_loss(rgb_pr, rgb_gt, reduction='none', beta=0.25), -1)
    return torch.sqrt(torch.sum((rgb_gt - rgb_pr) ** 2, dim=-1) + 0.001)


def shape_loss(kind, rgb, gt, gerr, eik_w, occ, cand, counts, gt_occ, w, dtype=F64):
    """losses [4] = (total, mean loss_rgb, mean(gerr * eik_w) * w[0], F.l1_loss(occ[cand[:kept]], gt_occ[:kept]) * w[1]) (train/trainer.py:127-137,
    network/loss.py) and d total / d (rgb, gerr, occ) by autograd.  No inner sample: no eikonal term; no kept candidate: no occlusion term."""
    a, b, c = leaf(rgb, dtype), leaf(gerr, dtype), leaf(occ, dtype)
    w0, w1 = (1.0, 1.0) if w is None else w
    zero = torch.zeros((), dtype=dtype)
    l_rgb = rgb_loss(kind, a, gt.to(dtype)).mean()
    l_eik = (b * eik_w).mean() * w0 if b.numel() else zero
    kept = 0 if cand is None else int(counts[0])
    l_occ = F.l1_loss(c[cand[:kept].long()], gt_occ[:kept].to(dtype)) * w1 if kept else zero
    total = l_rgb + l_eik + l_occ
    gs = torch.autograd.grad(total, [a, b, c], allow_unused=True)
    d_rgb, d_gerr, d_occ = [torch.zeros_like(t) if g_ is None else g_ for t, g_ in zip((a, b, c), gs)]
    return torch.stack([total, l_rgb, l_eik, l_occ]).detach(), d_rgb, d_gerr, d_occ


@functools.lru_cache(maxsize=None)
def loss_refs(R, n_in, mode, kind, wi, dtype=F64):
    q = loss_inputs(R, n_in, mode)
    return shape_loss(kind, q['rgb'], q['gt'], q['gerr'], EIK_W, q['occ'], q['cand'], q['counts'], q['gt_occ'], WEIGHTS[wi], dtype=dtype)


def loss_bounds(R, n_in, mode):
    """relative bounds of (total, loss_rgb, loss_eikonal, loss_occ) against float64; a term that is absent is exactly 0 and has none"""
    kept = {'none': 0, 'kept0': 0, 'kept1': 1, 'full': LOSS_CAP}[mode]
    terms = [loss_bound(R), loss_bound(n_in) if n_in else 0.0, loss_bound(kept) if kept else 0.0]
    return [max(terms) + 2 * EPS32] + terms


@functools.lru_cache(maxsize=None)
def loss_floors(kind):
    """the float32 floor of d_rgb / d_gerr / d_occ of one rgb kind over all shapes, occlusion modes and weights"""
    out = {'d_rgb': 0.0, 'd_gerr': 0.0, 'd_occ': 0.0}
    for R, n_in, mode in loss_family():
        for wi in range(len(WEIGHTS)):
            r64, r32 = loss_refs(R, n_in, mode, kind, wi), loss_refs(R, n_in, mode, kind, wi, F32)
            for i, nm in enumerate(('d_rgb', 'd_gerr', 'd_occ')):
                out[nm] = max(out[nm], row_err(r32[i + 1], r64[i + 1]))
    return out


# ---- nero_var_grad ------------------------------------------------------------------------------------------------------------------------
GATE = math.log(1e6) / 10                                                       # |variance| beyond it: inv_s leaves [1e-6, 1e6], no gradient
VARIANCES = tuple(np.float32(v) for v in list(np.linspace(-1.3, 1.3, 63)) + [0.3])          # 64 of them, 0.3 (the initial value) among them
GATE_VARIANCES = ((np.float32(1.39), False), (np.float32(-1.39), False), (np.float32(1.38), True), (np.float32(-1.38), True))   # (value, live)
DSUMS = (float(np.float32(0.37)), float(np.float32(-2.6)))


def var_grad(dsum, variance, dtype=F64):
    """dsum * d / d variance of exp(10 variance).clip(1e-6, 1e6) (network/field.py:192, network/renderer.py:491) by autograd"""
    v = leaf(torch.as_tensor(variance, dtype=F32).reshape(-1), dtype)
    inv_s = torch.exp(v * 10.0).clip(1e-6, 1e6)
    g, = torch.autograd.grad(inv_s.sum(), v)
    return g * torch.as_tensor(dsum, dtype=F32).to(dtype)


def var_grad_inputs():
    """-> variance [136], dsum [136]: every variance (the gate's four included) with a dsum of either sign"""
    v = [float(x) for x in VARIANCES] + [float(x) for x, _ in GATE_VARIANCES]
    return torch.tensor([x for x in v for _ in DSUMS], dtype=F32), torch.tensor([s for _ in v for s in DSUMS], dtype=F32)


@functools.lru_cache(maxsize=None)
def var_grad_floor():
    v, s = var_grad_inputs()
    return row_err(var_grad(s, v, F32), var_grad(s, v))
