"""Plain torch restatement of the kernels that turn gradients into the parameter update (nero_amd/csrc/trainer.hip: wn_forward_kernel,
wn_backward_kernel, wn_adam_kernel, adam_kernel; nero_amd/csrc/mlp_engine.hip: head_dw_kernel + head_dw_reduce_kernel), with no device code:
every function runs in the dtype of its tensors, float64 for the reference and float32 for the measured floor.  Pinned against
torch._weight_norm, torch.optim.Adam and einsum by tests/test_trainer_ref_cpu.py; the GPU tier is tests/test_trainer_kernels_gpu.py.

Term sizes (`unit`s, always float64): an output that is a signed sum is measured against the larger of its own magnitude and the sum of the
absolute values of its terms, which float32 cannot beat in any summation order:
  dg      : sum|dW v| inv_norm                                   dv : |g inv_norm| (|dW| + sum|dW v| inv_norm^2 |v|)
  Adam m  : the first moment of |grad| (of the gradient's own unit for a weight-norm job) under the same beta1
  Adam v  : the second moment of that unit (the plain jobs' v is a sum of squares: its own magnitude)
  update  : lr / bc1 x (unit of m) / denom                        p  : |p0| + the sum of the update units so far
  dWh     : sum_r |dy a| (+ sum_r |extra| in row 0)               dbh: sum_r |dy|

lr, the betas and eps cross the C ABI as floats: HYPERS holds their float32-rounded values, and the bias corrections are formed in double
from those, as the host code does.  `wrong`: the name of one deliberately wrong variant (WRONG below) -- the CPU tier feeds each through the
judge of the GPU tier and requires that it is rejected."""
import functools

import torch

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24
MAX_WN_JOBS, MAX_ADAM_JOBS = 40, 96

WRONG = ('eps_before_scale', 'call_step_for_own', 'dv_no_projection', 'dg_no_inv_norm', 'c2_inv_first_power', 'betas_swapped', 'v_from_g',
         'extra_every_row')
ADAM_WRONG = ('eps_before_scale', 'call_step_for_own', 'betas_swapped', 'v_from_g')
WN_WRONG = ('dv_no_projection', 'dg_no_inv_norm', 'c2_inv_first_power')


def c_float(x):
    """the value a C float parameter carries"""
    return float(torch.tensor(float(x), dtype=F32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- weight norm ---------------------------------------------------------------------------------------------------------------------------
def wn_forward(v, g):
    """v [rows, cols], g [rows] -> (w_eff = g v / ||v||_row, inv_norm = 1 / ||v||_row)"""
    n = (v * v).sum(-1).sqrt()
    return v * (g / n)[:, None], 1.0 / n


def wn_backward(v, g, inv_norm, dW, wrong=''):
    """-> dv, dg, unit of dv [rows, cols], unit of dg [rows] (units in float64)"""
    s = (dW * v).sum(-1)
    dg = s if wrong == 'dg_no_inv_norm' else s * inv_norm
    c1 = g * inv_norm
    c2 = s * inv_norm if wrong == 'c2_inv_first_power' else s * inv_norm * inv_norm
    dv = c1[:, None] * (dW if wrong == 'dv_no_projection' else dW - c2[:, None] * v)
    v_, g_, i_, d_ = v.double(), g.double(), inv_norm.double(), dW.double()
    S = (d_ * v_).abs().sum(-1)
    return dv, dg, (g_ * i_).abs()[:, None] * (d_.abs() + (S * i_ * i_)[:, None] * v_.abs()), S * i_


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, m, v, grad, lr, b1, b2, eps, step, job_step=0, wrong='', carry=None, gunit=None):
    """One torch.optim.Adam step in the operation order of trainer.hip's header:
        m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
    step: the call's 1-based step.  job_step (an int, or an int64 tensor per element): 0 = the call's step, > 0 = the job's own step,
    < 0 = no gradient: parameter and moments untouched.  carry: the running term sizes {'m', 'v', 'p'} of the previous step (None: the
    first); gunit: the unit of `grad` where it is itself a difference (default |grad|).  -> p, m, v, carry (carry only in float64)"""
    dt = p.dtype
    js = torch.as_tensor(job_step, dtype=torch.int64)
    own, skip = js > 0, (js < 0).expand(p.shape)
    eff = torch.full_like(js, int(step)) if wrong == 'call_step_for_own' else torch.where(own, js, torch.full_like(js, int(step)))
    if wrong == 'betas_swapped':
        b1, b2 = b2, b1
    bc1 = 1.0 - torch.tensor(b1, dtype=F64) ** eff.double()
    bc2 = 1.0 - torch.tensor(b2, dtype=F64) ** eff.double()
    step_size, inv_sqrt_bc2 = (lr / bc1).to(dt), (1.0 / bc2.sqrt()).to(dt)
    m1 = m + (grad - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * (grad if wrong == 'v_from_g' else grad * grad)
    denom = (v1.sqrt() + eps) * inv_sqrt_bc2 if wrong == 'eps_before_scale' else v1.sqrt() * inv_sqrt_bc2 + eps
    p1 = p - step_size * (m1 / denom)
    out = [torch.where(skip, a, b) for a, b in ((p, p1), (m, m1), (v, v1))]
    if dt != F64:
        return (*out, None)
    if carry is None:
        carry = dict(m=m.abs(), v=v.abs(), p=p.abs())
    U = grad.abs() if gunit is None else gunit
    mu = carry['m'] + (U - carry['m']) * (1.0 - b1)
    vu = b2 * carry['v'] + (1.0 - b2) * U * U
    pu = carry['p'] + step_size * mu / denom
    new = dict(m=torch.where(skip, carry['m'], mu), v=torch.where(skip, carry['v'], vu), p=torch.where(skip, carry['p'], pu))
    return (*out, new)


def wn_adam_step(v, g, inv_norm, dW, mv, vv, mg, vg, lr, b1, b2, eps, step, wrong='', carry=None):
    """weight-norm backward from the PRE-update (g, v) and the forward's inv_norm, then Adam on both.
    -> (v, mv, vv), (g, mg, vg), carry {'v': ..., 'g': ...}"""
    dv, dg, dvu, dgu = wn_backward(v, g, inv_norm, dW, wrong)
    carry = carry or dict(v=None, g=None)
    *nv, cv = adam_step(v, mv, vv, dv, lr, b1, b2, eps, step, 0, wrong, carry['v'], dvu)
    *ng, cg = adam_step(g, mg, vg, dg, lr, b1, b2, eps, step, 0, wrong, carry['g'], dgu)
    return tuple(nv), tuple(ng), dict(v=cv, g=cg)


# ---- head weight gradient ----------------------------------------------------------------------------------------------------------------
def head_dw(dy, a, extra, n_head, k_cols, wrong=''):
    """dy [rows, 4], a [rows, 256], extra [rows, 256] or None -> dWh [n_head, k_cols], dbh [n_head], and their units (float64)"""
    d, x = dy[:, :n_head], a[:, :k_cols]
    dWh, dbh = d.t() @ x, d.sum(0)
    uW, ub = d.double().abs().t() @ x.double().abs(), d.double().abs().sum(0)
    if extra is not None:
        e = extra[:, :k_cols].sum(0)
        rows = slice(0, n_head if wrong == 'extra_every_row' else 1)
        dWh = dWh.clone()
        dWh[rows] = dWh[rows] + e
        uW[0] = uW[0] + extra[:, :k_cols].double().abs().sum(0)
    return dWh, dbh, uW, ub


# ---- case tables -----------------------------------------------------------------------------------------------------------------------------
WN_ROWS = (1, 3, 4, 5, 217, 257)                                            # four rows share a block
WN_COLS = (1, 39, 63, 64, 65, 256, 259, 295)                                # the 64-lane stride
WN_SHAPES = tuple((r, c) for r in WN_ROWS for c in WN_COLS)
# a full batch with unequal rows: the grid is sized for the 257-row job, the surplus blocks of the others fall through
WN_BATCH = tuple((WN_ROWS[(5 * i) % 6], WN_COLS[(3 * i + i // 8) % 8]) for i in range(MAX_WN_JOBS))


@functools.lru_cache(maxsize=None)
def wn_inputs(rows, cols, seed=0):
    """v rows spread over several orders of magnitude, g of either sign, dW elements spread over e^(+-3) inside a row"""
    g = _gen(1000 * rows + cols + 7919 * seed)
    v = torch.randn(rows, cols, generator=g) * torch.exp(3.0 * torch.randn(rows, 1, generator=g))
    gg = (0.5 + torch.rand(rows, generator=g)) * (1.0 - 2.0 * (torch.rand(rows, generator=g) < 0.3).float())
    dW = 1e-3 * torch.randn(rows, cols, generator=g) * torch.exp(6.0 * torch.rand(rows, cols, generator=g) - 3.0)
    return dict(v=v, g=gg, dW=dW)


# hyper-parameters (lr, beta1, beta2, eps) as C floats: the product's betas and eps, and one set where nothing is at its default
HYPERS = tuple(tuple(c_float(x) for x in h) for h in ((5e-4, 0.9, 0.999, 1e-8), (1e-2, 0.5, 0.9, 1e-3)))
FIRST_STEPS = (1, 25000)                                                    # the bias corrections at their largest, and next to 1
P_SCALES = (0.0, 1.0)                                                       # p shows the accumulated update at full precision / unit scale
N_CALLS = 8
PLAIN_N = (1, 255, 256, 257, 16384, 16385, 70001)                           # the 256-thread block, the 64-block cap (64 x 256) and its stride
GRAD_CLASSES = ('wide', 'zero', 'tiny', 'eps', 'unit')


def draw_grad(n, call, g):
    """a fresh gradient: blocks of seven elements cycle through the magnitude classes, shifted by the call so that a one-element tensor
    meets each: 'wide' +-e^(-8 +- 6), exact zeros, +-1e-12, eps-sized +-1e-8 x [0.1, 10], and unit normal"""
    sign = 1.0 - 2.0 * (torch.rand(n, generator=g) < 0.5).float()
    u, z = torch.rand(n, generator=g), torch.randn(n, generator=g)
    cls = (torch.arange(n) // 7 + call) % len(GRAD_CLASSES)
    out = sign * torch.exp(-8.0 + 6.0 * (2.0 * u - 1.0))
    out = torch.where(cls == 1, torch.zeros(n), out)
    out = torch.where(cls == 2, sign * 1e-12, out)
    out = torch.where(cls == 3, sign * 1e-8 * torch.exp(2.302585 * (2.0 * u - 1.0)), out)
    return torch.where(cls == 4, z, out)


def _plain_sizes(n_plain, big):
    small = (1, 2, 3, 5, 7, 17, 64, 65)
    sizes = [small[i % len(small)] for i in range(n_plain)]
    for k, n in enumerate(big):                                             # tiny and large tensors mixed in one call
        sizes[(k * 37 + 1) % n_plain if n_plain > 1 else 0] = n
    return tuple(sizes)


def _plain_kinds(n_plain):
    """job -> 'call' (step 0), 'late' (no gradient for three calls, then its own step 1, 2, ...), 'never' (no gradient at all), 'own' (its own
    step from the first call on): both sides of the 96-job chunk boundary where there is one"""
    kinds = ['call'] * n_plain
    marks = {93: 'own', 94: 'never', 95: 'late', 96: 'late', 97: 'never', 98: 'own'} if n_plain > MAX_ADAM_JOBS else {1: 'late', 2: 'never', 3: 'own'}
    for i, k in marks.items():
        if i < n_plain and n_plain > 1:
            kinds[i] = k
    return tuple(kinds)


def job_step_of(kind, call):
    return {'call': 0, 'never': -1, 'own': call + 1, 'late': -1 if call < 3 else call - 2}[kind]


# one case per (hyper set, first step, p scale); over the eight: n_plain in {1, 96, 97, 200} and 0, n_wn = 0, every PLAIN_N
ADAM_CASES = (
    dict(hyper=0, step0=1, pscale=0.0, wn=((3, 39), (5, 64), (217, 65), (4, 259)), plain=PLAIN_N),
    dict(hyper=1, step0=1, pscale=1.0, wn=(), plain=_plain_sizes(200, (16385, 70001))),
    dict(hyper=0, step0=25000, pscale=1.0, wn=((1, 63), (257, 39), (5, 295)), plain=()),
    dict(hyper=1, step0=25000, pscale=0.0, wn=((4, 65), (3, 256)), plain=_plain_sizes(97, (257, 16384))),
    dict(hyper=0, step0=1, pscale=1.0, wn=((5, 39),), plain=_plain_sizes(96, (255, 256))),
    dict(hyper=1, step0=1, pscale=0.0, wn=((217, 64), (1, 259)), plain=(70001,)),
    dict(hyper=0, step0=25000, pscale=0.0, wn=(), plain=_plain_sizes(200, (1, 16385))),
    dict(hyper=1, step0=25000, pscale=1.0, wn=((3, 65), (4, 39)), plain=(1,)),
)


def _init_state(shape, pscale, warm, g):
    """p at `pscale`; zero moments at a first step of 1, else the moments of a run in progress"""
    p = pscale * torch.randn(shape, generator=g)
    if not warm:
        return p, torch.zeros(shape), torch.zeros(shape)
    s = torch.exp(-6.0 + 3.0 * torch.randn(shape, generator=g))
    return p, 0.3 * s * torch.randn(shape, generator=g), s * s * (0.5 + torch.rand(shape, generator=g))


@functools.lru_cache(maxsize=None)
def adam_case_inputs(ci):
    """the float32 inputs of ADAM_CASES[ci]: initial state and the gradient of every call, for the flat concatenation of the plain jobs
    and for each weight-norm job"""
    c, g = ADAM_CASES[ci], _gen(4242 + ci)
    warm = c['step0'] > 1
    N = sum(c['plain'])
    plain = dict(zip('pmv', _init_state((N,), c['pscale'], warm, g)))
    plain['grads'] = [draw_grad(N, k, g) for k in range(N_CALLS)]
    plain['job'] = torch.repeat_interleave(torch.arange(len(c['plain'])), torch.tensor(c['plain'], dtype=torch.int64)) if N else torch.zeros(0, dtype=torch.int64)
    plain['kinds'] = _plain_kinds(len(c['plain']))
    wn = []
    for rows, cols in c['wn']:
        w = wn_inputs(rows, cols, seed=1 + ci)
        # (a zero v has no norm: the weight-norm jobs start from wn_inputs in every case; the rows of v span e^(+-9), and the small ones
        # show an update whole)
        v, gg = w['v'], w['g']
        _, mv, vv = _init_state((rows, cols), 0.0, warm, g)
        _, mg, vg = _init_state((rows,), 0.0, warm, g)
        dWs = [draw_grad(rows * cols, k, g).reshape(rows, cols) for k in range(N_CALLS)]
        wn.append(dict(v=v, g=gg, mv=mv, vv=vv, mg=mg, vg=vg, dWs=dWs, rows=rows, cols=cols))
    return dict(plain=plain, wn=wn, hyper=HYPERS[c['hyper']], step0=c['step0'])


def plain_job_steps(inp, call):
    """per job, and per element of the flat concatenation"""
    js = torch.tensor([job_step_of(k, call) for k in inp['plain']['kinds']], dtype=torch.int64)
    return js, js[inp['plain']['job']] if js.numel() else js


ADAM_OUT = ('plain.p', 'plain.m', 'plain.v', 'wn.v', 'wn.m_v', 'wn.v_v', 'wn.g', 'wn.m_g', 'wn.v_g')
WN_KEYS = ('v', 'mv', 'vv', 'g', 'mg', 'vg')                               # a weight-norm job's state, in the order of ADAM_OUT[3:]


def wn_call_refs(state, inv_norm, dW, hyper, step):
    """ONE fused call on a weight-norm job's own float32 state (WN_KEYS), the inv_norm its forward left and its float32 dW
    -> state key -> (float64 reference, float32 reference, unit).  The units are those of a first step: the moments and the parameter the
    call was handed are its exact inputs.  (A weight-norm job is judged call by call on the state it is really in, not against a float64
    trajectory of its own: dv depends on v, and a parameter that eight updates of alternating sign have brought back near its start is known
    only to a rounding of those updates, far more than a rounding of itself -- measured here: 30 roundings of m_v after eight calls.)"""
    res = {}
    for dt in (F64, F32):
        s = {k: state[k].to(dt) for k in WN_KEYS}
        nv, ng, carry = wn_adam_step(s['v'], s['g'], inv_norm.to(dt), dW.to(dt), s['mv'], s['vv'], s['mg'], s['vg'], *hyper, step)
        res[dt] = dict(zip(WN_KEYS, (*nv, *ng)))
        if dt == F64:
            cv, cg = carry['v'], carry['g']
            unit = dict(v=cv['p'], mv=cv['m'], vv=cv['v'], g=cg['p'], mg=cg['m'], vg=cg['v'])
    return {k: (res[F64][k], res[F32][k], unit[k]) for k in WN_KEYS}


def adam_trajectory(ci, dt, wrong=''):
    """N_CALLS consecutive calls of ADAM_CASES[ci].  The plain jobs in `dt` (their gradients are inputs: the float64 run IS the reference of
    every call) -> per call {'plain.p' / 'plain.m' / 'plain.v': tensor}, and (float64 only) the running units in the same layout.
    The weight-norm jobs only in float32, as the candidate a judge is handed: each runs its own forward before every call, as the trainer
    does, and every call adds 'wn.*': the candidate's new state per job, and 'wn_refs': wn_call_refs of the state it was in."""
    inp = adam_case_inputs(ci)
    hyper = inp['hyper']
    pl = inp['plain']
    p, m, v = (pl[k].to(dt) for k in 'pmv')
    carry = None
    wn = [{k: w[k] for k in WN_KEYS} for w in inp['wn']] if dt == F32 else []
    outs, units = [], []
    for call in range(N_CALLS):
        step = inp['step0'] + call
        o, u = {}, {}
        if p.numel():
            p, m, v, carry = adam_step(p, m, v, pl['grads'][call].to(dt), *hyper, step, plain_job_steps(inp, call)[1], wrong, carry)
            o.update({'plain.p': p, 'plain.m': m, 'plain.v': v})
            if carry is not None:
                u.update({'plain.p': carry['p'], 'plain.m': carry['m'], 'plain.v': carry['v']})
        if wn:
            o['wn_refs'] = []
            for k in ADAM_OUT[3:]:
                o[k] = []
        for j, (s, w) in enumerate(zip(wn, inp['wn'])):
            inv, dW = wn_forward(s['v'], s['g'])[1], w['dWs'][call]
            refs = wn_call_refs(s, inv, dW, hyper, step)
            if wrong:
                nv, ng, _ = wn_adam_step(s['v'], s['g'], inv, dW, s['mv'], s['vv'], s['mg'], s['vg'], *hyper, step, wrong)
                wn[j] = dict(zip(WN_KEYS, (*nv, *ng)))
            else:
                wn[j] = {k: refs[k][1] for k in WN_KEYS}
            o['wn_refs'].append(refs)
            for name, k in zip(ADAM_OUT[3:], WN_KEYS):
                o[name].append(wn[j][k])
        outs.append(o)
        units.append(u)
    return outs, units


def flat(x):
    """a tensor, or a list of tensors per job -> one element per row"""
    if isinstance(x, (list, tuple)):
        return torch.cat([t.reshape(-1) for t in x]) if x else torch.zeros(0)
    return x.reshape(-1)


@functools.lru_cache(maxsize=None)
def adam_refs(ci):
    """-> (float64 plain trajectory, the float32 candidate of the correct formulas, plain units): computed once, shared, not modified"""
    r64, units = adam_trajectory(ci, F64)
    return r64, adam_trajectory(ci, F32)[0], units


def call_refs(ci, call, name, cand=None):
    """(float64 reference, float32 reference, unit) of output `name` after call `call`: a plain output from the trajectories, a
    weight-norm output from the state the candidate `cand` (default: the correct float32 one) was in before the call"""
    r64, r32, units = adam_refs(ci)
    if name.startswith('plain.'):
        return r64[call][name], r32[call][name], units[call][name]
    k = WN_KEYS[ADAM_OUT[3:].index(name)]
    refs = (r32 if cand is None else cand)[call]['wn_refs']
    return tuple([r[k][i] for r in refs] for i in range(3))


def call_outputs(ci):
    """the outputs ADAM_CASES[ci] has after every call"""
    c = ADAM_CASES[ci]
    return (ADAM_OUT[:3] if c['plain'] else ()) + (ADAM_OUT[3:] if c['wn'] else ())


# head gradient
HEAD_ROWS = (0, 1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 300, 512, 513, 128 * 16 + 1, 33000)   # 512 / 513: four and five slices
HEAD_K = (1, 39, 128, 256)
HEAD_N = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def head_inputs(rows):
    g = _gen(77 + rows)
    dy = torch.randn(rows, 4, generator=g) * torch.exp(2.0 * torch.randn(rows, 1, generator=g))
    a = torch.relu(torch.randn(rows, 256, generator=g) + 0.3) * torch.exp(torch.randn(1, 256, generator=g))
    return dict(dy=dy, a=a, extra=0.3 * torch.randn(rows, 256, generator=g))


@functools.lru_cache(maxsize=None)
def head_refs(rows, with_extra):
    """the full [4, 256] problem once per row count -> {dtype: (dWh, dbh)}, unit of dWh, unit of dbh; every (n_head, k_cols) case is a
    slice of it (row j of dWh depends on column j of dy alone, column k on column k of a alone)"""
    h = head_inputs(rows)
    out = {}
    for dt in (F64, F32):
        dWh, dbh, uW, ub = head_dw(h['dy'].to(dt), h['a'].to(dt), h['extra'].to(dt) if with_extra else None, 4, 256)
        out[dt] = (dWh, dbh)
    return out, uW, ub
