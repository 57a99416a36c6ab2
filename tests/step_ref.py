"""The comparison that pins the two decode-step kernels of csrc/step.hip
(mtts.ops.state_update, mtts.ops.conv_update), shared by
tests/test_step_ref_cpu.py (which proves it on the CPU: the references against
the sequence oracle, the bound against a float32 evaluation and against the
listed mutants) and tests/test_gpu_step.py (which checks the kernels against it).

`state_reference`, `conv_reference`: float64, oracle.mamba_ref's
selective_state_update_ref / causal_conv1d_update_ref on exactly the values the
kernel reads (bf16 inputs upcast; the fused dt = x_dbl[:, :R] @ dt_w.T formed
in float64).  Beside each output they return a condition number per element.

The state update, with eps = 2^-24 (one fp32 rounding):
    p   = dt_raw + dt_bias;   dt = softplus(p) or p;   a = dt A
    e   = exp(a);   h' = e h + dt x B;   y = (sum_i C_i h'_i + D x) silu(z)
Errors of an fp32 evaluation, to first order:
  * dt.  The fused dot of R products carries at most R eps sum|x_r w_r|
    (d_dot); a given dt is exact (d_dot = 0).  p is rounded once, eps |p|,
    and so is the argument of the exponential inside softplus, which moves its
    result by the same eps |p| softplus'(p); softplus' = sigmoid(p) <= 1
    scales both, and the result is rounded again:
        d_dt = s' (d_dot + eps |p|) + eps |dt|,    s' = sigmoid(p) or 1.
    This asks for a softplus that is accurate RELATIVE to its result; one that
    forms log(1 + e^p) with the sum rounded to fp32 is accurate to eps
    absolutely, 1000 eps relatively at dt = 1e-3 (mutant "softplus_log_1_plus").
  * e.  The argument a (and a log2(e) where exp2 is used) is rounded:
    eps |a| absolute in the argument is eps |a| relative in e; exp and the
    product e h add a rounding each: (1 + |a|) |e h| eps, constants left to k.
  * dt x B: a rounding per product, |dt x B| eps.
  * d_dt reaches h' through dh'/d dt = A e h + x B.
        cond_h = (1 + |dt A|) |e h| + |dt x B| + d_dt (|A e h| + |x B|) / eps
  * y sums 16 products of h' (|h'_i| <= cond_h_i) and D x, then scales:
        cond_y = (sum_i |C_i| cond_h_i + |D x|) |silu(z)|
    (the D term and the silu factor drop out when absent).
The criterion is elementwise, |got - ref| <= K eps cond + floor, plus
2^-8 |ref| where the output is stored as bf16.  `floor` is the smallest normal
fp32 number, 2^-126 (times 1 + sum_i |C_i| |silu(z)| for y): the kernels flush
denormals, so exp(-100), silu(-100) and their products come out as 0.

The conv update: window' = [window[1:], x] (bit for bit: fp32 copies of the
inputs), v = sum_k w_k window'_k + bias, out = silu(v) or v.
        cond_v = sum_k |w_k window'_k| + |bias|
        cond_out = cond_v |silu'(v)| + |out|,   silu'(v) = s (1 + v (1 - s))
(the |out| term is the rounding of the result and of the sigmoid's argument).

`state_float32`, `conv_float32`: the same formulas in float32 torch on the CPU,
outputs rounded to the I/O dtype, with the mutants the criterion must reject.

K is measured, not chosen: tests/test_gpu_step.py's docstring has the table."""
import functools
import itertools
import types
import zlib

import torch
import torch.nn.functional as F

from oracle import mamba_ref as R

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = 2.0 ** -24
TINY = 2.0 ** -126
BF16_ULP = 2.0 ** -8
K = 16.0
N = 16
TAG = {F32: "f32", BF16: "bf16"}
LOG2E = 1.4426950408889634


# ------------------------------------------------------------------ the cases
STATE_SHAPES = [(1, 1), (3, 7), (5, 96), (3, 80), (33, 64)]
DTYPE_PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
OPTIONS = [dict(zip(("D", "z", "bias", "softplus"), bits)) for bits in itertools.product((True, False), repeat=4)]
FUSED_RANKS = [1, 3, 4, 7, 8, 9, 32, 48, 64, 160]
FUSED_SHAPE = (5, 96)
PRE_SOFTPLUS = [-30.0, -7.0, 19.999, 20.0, 20.001, 60.0]
EDGES = [f"pre_softplus_{v:g}" for v in PRE_SOFTPLUS] + ["exp_underflow", "x_zero", "z_minus_100", "z_plus_100",
                                                           "zero_state", "negative_dt"]
EDGE_SHAPE = (2, 24)
CONV_SHAPES = [(1, 1), (3, 7), (5, 96), (2, 2048), (33, 100)]
CONV_OPTIONS = [dict(bias=b, silu=s) for b in (True, False) for s in (True, False)]


def opt_name(o):
    return "+".join(k for k, v in o.items() if v) or "none"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def inv_softplus(t):
    return t + torch.log(-torch.expm1(-t))


@functools.lru_cache(maxsize=None)
def state_inputs(B, D, io=F32, bc=F32, has_D=True, has_z=True, has_bias=True, softplus=True, rank=0, edge=None):
    """CPU tensors in the dtypes the kernel is given.  Steps as a trained layer
    has them: with softplus and a bias, softplus(dt_bias) is log-uniform in
    [1e-3, 1e-1] (mamba-ssm's initialisation) under a unit-normal dt; without
    softplus the step itself is positive, 1e-3 to 0.1."""
    g = _gen(B, D, TAG[io], TAG[bc], has_D, has_z, has_bias, softplus, rank, edge)
    rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)            # noqa: E731
    i = types.SimpleNamespace(io=io, bc=bc, softplus=softplus, rank=rank, dt_w=None)
    i.state, i.x = rn(B, D, N), rn(B, D).to(io)
    i.A = -(0.5 + 15.5 * ru(D, N))
    i.Bm, i.Cm = rn(B, N).to(bc), rn(B, N).to(bc)
    i.D = rn(D) if has_D else None
    i.z = rn(B, D).to(io) if has_z else None
    if softplus:
        i.dt_bias = inv_softplus(torch.exp(ru(D) * 4.605 - 6.908)) if has_bias else None
        dt = rn(B, D)
    else:
        i.dt_bias = 0.01 * ru(D) if has_bias else None
        dt = 1e-3 + 0.1 * ru(B, D)
    if rank:
        i.dt = rn(B, rank).to(io)
        i.dt_w = (rn(D, rank) / rank ** 0.5).to(io)
    else:
        i.dt = dt.to(io)
    if edge is not None:
        _edge(i, edge, B, D)
    return i


def _edge(i, edge, B, D):
    assert i.io == F32 and not i.rank
    if edge.startswith("pre_softplus_"):
        i.dt_bias = torch.full((D,), 0.5)
        i.dt = torch.full((B, D), float(edge[len("pre_softplus_"):])) - 0.5
        if i.dt[0, 0] > 10:        # a step this long with A ~ -8 would underflow every state
            i.A = -(1e-3 + 1e-2 * torch.rand(D, N, generator=_gen(edge)))
    elif edge == "exp_underflow":  # dt A in [-160, -95]
        i.softplus, i.dt_bias = False, None
        i.dt = torch.full((B, D), 10.0)
        i.A = i.A.clamp(max=-9.5)
    elif edge == "x_zero":
        i.x = torch.zeros(B, D)
    elif edge == "z_minus_100":
        i.z = torch.full((B, D), -100.0)
    elif edge == "z_plus_100":
        i.z = torch.full((B, D), 100.0)
    elif edge == "zero_state":
        i.state = torch.zeros(B, D, N)
    elif edge == "negative_dt":
        i.softplus, i.dt_bias = False, None
        i.dt = -(0.05 + 0.45 * torch.rand(B, D, generator=_gen(edge)))
    else:
        raise KeyError(edge)


def edge_inputs(edge):
    return state_inputs(*EDGE_SHAPE, edge=edge)


@functools.lru_cache(maxsize=None)
def conv_inputs(B, D, io=F32, has_bias=True, silu=True):
    g = _gen("conv", B, D, TAG[io], has_bias, silu)
    rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
    return types.SimpleNamespace(io=io, silu=silu, x=rn(B, D).to(io), conv_state=rn(B, D, 4), w=0.5 * rn(D, 4),
                                 bias=rn(D) if has_bias else None)


# ----------------------------------------------------------- float64 references
def _d(t):
    return None if t is None else t.to(F64)


def state_reference(i):
    """{"state", "y", "cond_h", "cond_y", "floor_y"}: float64, see the module docstring."""
    x, A, Bm, Cm, h = _d(i.x), _d(i.A), _d(i.Bm), _d(i.Cm), _d(i.state)
    if i.dt_w is not None:
        dt_raw = _d(i.dt) @ _d(i.dt_w).t()
        d_dot = i.dt.shape[1] * EPS * (_d(i.dt).abs() @ _d(i.dt_w).abs().t())
    else:
        dt_raw, d_dot = _d(i.dt), 0.0
    y, new = R.selective_state_update_ref(h, x, dt_raw, A, Bm, Cm, _d(i.D), _d(i.z), _d(i.dt_bias), i.softplus)
    p = dt_raw if i.dt_bias is None else dt_raw + _d(i.dt_bias)[None]
    dt = R.softplus(p) if i.softplus else p
    slope = torch.where(p <= 20.0, torch.sigmoid(p), torch.ones_like(p)) if i.softplus else 1.0
    d_dt = slope * (d_dot + EPS * p.abs()) + EPS * dt.abs()
    a = dt[..., None] * A[None]
    eh = (torch.exp(a) * h).abs()
    xB = (x[..., None] * Bm[:, None, :]).abs()
    cond_h = (1 + a.abs()) * eh + dt.abs()[..., None] * xB + (d_dt / EPS)[..., None] * (A.abs()[None] * eh + xB)
    cond_y = (Cm.abs()[:, None, :] * cond_h).sum(-1)
    floor_y = Cm.abs().sum(-1, keepdim=True).expand_as(cond_y).clone()
    if i.D is not None:
        cond_y = cond_y + (_d(i.D)[None] * x).abs()
    if i.z is not None:
        cond_y, floor_y = cond_y * F.silu(_d(i.z)).abs(), floor_y * F.silu(_d(i.z)).abs()
    return {"state": new, "y": y, "cond_h": cond_h, "cond_y": cond_y, "floor_y": TINY * (1 + floor_y)}


def conv_reference(i):
    """{"out", "conv_state", "cond"}: float64; conv_state is exact in fp32."""
    out, st = R.causal_conv1d_update_ref(_d(i.x), _d(i.conv_state), _d(i.w), _d(i.bias), "silu" if i.silu else None)
    cond = (st * _d(i.w)[None]).abs().sum(-1)
    if i.bias is not None:
        cond = cond + _d(i.bias).abs()[None]
    if i.silu:
        v = (st * _d(i.w)[None]).sum(-1) + (0.0 if i.bias is None else _d(i.bias)[None])
        s = torch.sigmoid(v)
        cond = cond * (s * (1 + v * (1 - s))).abs() + out.abs()
    return {"out": out, "conv_state": st, "cond": cond}


# ------------------------------------------------------ the kernels in fp32 torch
STATE_MUTANTS = ("dropped_state", "softplus_log_1_plus")
CONV_MUTANTS = ("window_shifted",)


def state_float32(i, mutant=None):
    """csrc/step.hip's state update in float32 torch: (y in the I/O dtype, new state fp32)."""
    assert mutant is None or mutant in STATE_MUTANTS
    f = lambda t: None if t is None else t.float()        # noqa: E731
    x, A, Bm, Cm, h = f(i.x), i.A, f(i.Bm), f(i.Cm), i.state
    dt = f(i.dt) @ f(i.dt_w).t() if i.dt_w is not None else f(i.dt)
    if i.dt_bias is not None:
        dt = dt + i.dt_bias[None]
    if i.softplus:
        e = torch.exp(dt.clamp(max=20.0))
        sp = torch.log(1.0 + e) if mutant == "softplus_log_1_plus" else torch.log1p(e)
        dt = torch.where(dt > 20.0, dt, sp)
    e = torch.exp2(dt[..., None] * A[None] * LOG2E)
    new = e * h + (dt * x)[..., None] * Bm[:, None, :]
    n = N - 1 if mutant == "dropped_state" else N
    y = (Cm[:, None, :n] * new[..., :n]).sum(-1)
    if i.D is not None:
        y = y + i.D[None] * x
    if i.z is not None:
        y = y * (f(i.z) * torch.sigmoid(f(i.z)))
    return y.to(i.io), new


def conv_float32(i, mutant=None):
    """csrc/step.hip's conv update in float32 torch: (out in the I/O dtype, new window fp32)."""
    assert mutant is None or mutant in CONV_MUTANTS
    st = torch.cat([i.conv_state[:, :, 1:], i.x.float()[:, :, None]], -1)
    win = torch.roll(st, 1, -1) if mutant == "window_shifted" else st
    v = (win * i.w[None]).sum(-1)
    if i.bias is not None:
        v = v + i.bias[None]
    if i.silu:
        v = v * torch.sigmoid(v)
    return v.to(i.io), st


# ----------------------------------------------------------------- the criterion
def ratio(got, ref, cond, floor=TINY):
    """max over the elements of (|got - ref| - floor - 2^-8 |ref| if bf16) /
    (eps cond): the figure K bounds.  inf for a non-finite output, and where
    an element with cond = 0 is off by more than the floor."""
    got = got.detach().cpu()
    assert got.dtype in (F32, BF16), got.dtype
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got.double() - ref).abs() - floor
    if got.dtype == BF16:
        err = err - BF16_ULP * ref.abs()
    err = err.clamp_min(0.0)
    q = torch.where(err > 0, err / (EPS * cond), torch.zeros_like(err))    # x / 0 = inf
    return q.max().item() if q.numel() else 0.0


def state_ratios(y, state, ref):
    return {"y": ratio(y, ref["y"], ref["cond_y"], ref["floor_y"]),
            "state": ratio(state, ref["state"], ref["cond_h"])}


def check_state(y, state, ref, io, name="", k=None):
    """Assert the criterion on a state update's two outputs; returns the ratios."""
    k = K if k is None else k
    assert y.dtype == io and state.dtype == F32, (name, y.dtype, state.dtype)
    q = state_ratios(y, state, ref)
    assert all(v <= k for v in q.values()), f"{name}: err / (eps cond) = {q}, allowed {k}"
    return q


def check_conv(out, conv_state, ref, io, name="", k=None):
    k = K if k is None else k
    assert out.dtype == io and conv_state.dtype == F32, (name, out.dtype, conv_state.dtype)
    assert torch.equal(conv_state.detach().cpu().double(), ref["conv_state"]), f"{name}: window not bit-exact"
    q = ratio(out, ref["out"], ref["cond"])
    assert q <= k, f"{name}: err / (eps cond) = {q:.2f}, allowed {k}"
    return q
