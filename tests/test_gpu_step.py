"""The decode-step kernels of csrc/step.hip (conv_update_kernel,
state_update_kernel, through mtts.ops.conv_update / state_update) against the
float64 references of tests/step_ref.py, element by element:
    |got - ref| <= K 2^-24 cond + floor  (+ 2^-8 |ref| for a bf16 output)
with cond, floor and their derivation in step_ref's docstring, and
tests/test_step_ref_cpu.py showing that a float32 evaluation meets the bound
and that a dropped state, a shifted window and a softplus with a rounded sum
do not.  Every shape is tiny; the references are computed once per case.

K.  Largest err / (2^-24 cond) measured on an MI355X with the bound switched
off, per output and (io, bc) dtype pair, over every test of this file:

    io / bc       new state    y       conv out
    f32 / f32       1.71      2.32      2.66
    f32 / bf16      1.49      3.36       -
    bf16 / f32      1.51      0.19       -
    bf16 / bf16     1.61      0.00      0.00
  by family (state, y): options 1.71, 3.36; fused dt_proj 1.47, 1.99; tail
  lanes 1.27, 1.49; decode layout 1.34, 1.40; edge values 1.26, 2.10.
(A bf16 y or out is within its own rounding of the reference nearly
everywhere, hence the zeros; the fp32 state is what pins those kernels.)
K = 4 x the largest figure, rounded up to a power of two: 4 x 3.36 -> 16
(step_ref.K).  The float32 evaluation on the CPU stays below 2.8.

The same run on the kernel as it stood before this suite gave a new state of
up to 81.9 (f32 / f32; 80.0, 72.0, 57.6 for the other pairs) and y up to 9.2:
its softplus formed log(1 + e) with the sum rounded to fp32, which is eps
accurate absolutely and 10 to 1000 eps relatively at the steps a trained layer
takes.  step.hip now uses log1pf there (softplus_step); the figures above are
with it.

The prefill -> step hand-off runs 6 steps after a ragged prefill; errors
compound over steps and through the bf16 u between conv and scan, so that one
test uses test_gpu_ops.close() at the 1e-2 this file family uses for bf16."""
import types

import pytest
import torch

import step_ref as S
from oracle import mamba_ref as R
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = S.F32, S.BF16
PAIRS = [pytest.param(io, bc, id=f"{S.TAG[io]}-{S.TAG[bc]}") for io, bc in S.DTYPE_PAIRS]
IOS = [pytest.param(io, id=S.TAG[io]) for io in (F32, BF16)]
SHAPE_ID = lambda s: f"{s[0]}x{s[1]}"    # noqa: E731
SENTINEL = 7.0


def _dev(i):
    return types.SimpleNamespace(**{k: v.to(DEV) if torch.is_tensor(v) else v for k, v in vars(i).items()})


def _state_update(d, state=None, out=None, **over):
    """ops.state_update on the device copy `d` of a case; returns (y, state)."""
    from mtts import ops
    a = dict(vars(d), **over)
    st = a["state"].clone() if state is None else state
    y = ops.state_update(st, a["x"], a["dt"], a["A"], a["Bm"], a["Cm"], a["D"], a["z"], a["dt_bias"], a["softplus"],
                         out=out, dt_w=a["dt_w"])
    return y, st


def _conv_update(d, state=None, out=None, **over):
    from mtts import ops
    a = dict(vars(d), **over)
    st = a["conv_state"].clone() if state is None else state
    return ops.conv_update(a["x"], st, a["w"], a["bias"], a["silu"], out=out), st


def _opts(o):
    return dict(has_D=o["D"], has_z=o["z"], has_bias=o["bias"], softplus=o["softplus"])


def _report(what, io, bc, q):
    print(f"RATIO {what} {S.TAG[io]}/{S.TAG[bc]} " + " ".join(f"{k}={v:.3f}" for k, v in q.items()))


# ------------------------------------------------------- state_update vs float64
@pytest.mark.parametrize("io,bc", PAIRS)
@pytest.mark.parametrize("shape", S.STATE_SHAPES, ids=SHAPE_ID)
def test_state_update_vs_float64(shape, io, bc):
    """Every subset of {D, z, dt_bias, softplus} on a random non-zero state:
    the in-place state and y, element by element."""
    worst = {"y": 0.0, "state": 0.0}
    for o in S.OPTIONS:
        i = S.state_inputs(*shape, io, bc, **_opts(o))
        y, st = _state_update(_dev(i))
        q = S.check_state(y, st, S.state_reference(i), io, f"{shape} {S.opt_name(o)}")
        worst = {k: max(worst[k], q[k]) for k in q}
    _report(f"options {shape}", io, bc, worst)


@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (3, 80)], ids=SHAPE_ID)
def test_state_update_tail_lanes_store_nothing(shape, io):
    """The lanes past B * D compute on row 0 and must store nothing: the state
    is the first B rows of a (B + 2, D, 16) buffer, y a column view of a wider
    one, and everything outside the views is bit-identical afterwards."""
    B, D = shape
    i = S.state_inputs(B, D, io, io)
    d = _dev(i)
    big = torch.full((B + 2, D, S.N), SENTINEL, device=DEV)
    big[:B] = d.state
    wide = torch.full((B + 2, D + 9), SENTINEL, device=DEV, dtype=io)
    big0, wide0 = big.clone(), wide.clone()
    y, st = _state_update(d, state=big[:B], out=wide[:B, 4:4 + D])
    assert y.data_ptr() == wide[:B, 4:4 + D].data_ptr()
    _report(f"tail {shape}", io, io, S.check_state(y, st, S.state_reference(i), io))
    assert torch.equal(big[B:], big0[B:]), "a state store landed past row B"
    wide0[:B, 4:4 + D] = y
    assert torch.equal(wide, wide0), "a y store landed outside its view"


@pytest.mark.parametrize("io,rank", [pytest.param(io, r, id=f"{S.TAG[io]}-R{r}")
                                     for io, r in ((F32, 7), (BF16, 32), (BF16, 4), (F32, 64))])
def test_state_update_decode_layout(io, rank):
    """What decode.py passes: x = xz[:, :D], z = xz[:, D:], dt / B / C views of
    one x_dbl (B, R + 2N), dt_proj fused.  Bit for bit the run on contiguous
    copies, and within the bound."""
    B, D = 5, 96
    i = S.state_inputs(B, D, io, io, rank=rank)
    d = _dev(i)
    xz = torch.cat([d.x, d.z], 1)
    x_dbl = torch.cat([d.dt, d.Bm, d.Cm], 1)
    Nn = S.N
    views = dict(x=xz[:, :D], z=xz[:, D:], dt=x_dbl[:, :rank], Bm=x_dbl[:, rank:rank + Nn], Cm=x_dbl[:, rank + Nn:])
    assert not any(v.is_contiguous() for v in views.values())
    y1, s1 = _state_update(d, **views)
    y2, s2 = _state_update(d)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    _report(f"decode-layout R={rank}", io, io, S.check_state(y1, s1, S.state_reference(i), io))


@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("rank", S.FUSED_RANKS)
def test_state_update_fused_dt_proj_vs_float64(rank, io):
    """dt = x_dbl[:, :R] @ dt_w.T inside the kernel: the quad's strided scalar
    loop with its r + 4 < R tail, and for bf16 rows of R % 32 == 0 the 16-byte
    loads -- run once more with dt 4 elements into a wider row, which is not
    16-byte aligned and takes the scalar loop."""
    i = S.state_inputs(*S.FUSED_SHAPE, io, io, rank=rank)
    d, ref = _dev(i), S.state_reference(i)
    y, st = _state_update(d)
    _report(f"fused R={rank}", io, io, S.check_state(y, st, ref, io, f"R={rank}"))
    if io == BF16 and rank in (32, 64):
        wide = torch.zeros(d.dt.shape[0], rank + 8, device=DEV, dtype=io)
        wide[:, 4:4 + rank] = d.dt
        dt = wide[:, 4:4 + rank]
        assert dt.data_ptr() % 16 == 8
        y, st = _state_update(d, dt=dt)
        _report(f"fused R={rank} unaligned", io, io, S.check_state(y, st, ref, io, f"R={rank} unaligned"))


@pytest.mark.parametrize("edge", S.EDGES)
def test_state_update_edge_values(edge):
    """Both softplus branches and its threshold, exp2 underflow, x = 0,
    saturated gates, a zero state and a negative step without softplus: finite
    and within the bound."""
    i = S.edge_inputs(edge)
    y, st = _state_update(_dev(i))
    assert torch.isfinite(y).all() and torch.isfinite(st).all()
    _report(edge, F32, F32, S.check_state(y, st, S.state_reference(i), F32, edge))
    if edge == "exp_underflow":      # e is 0: the state is the rounded product and nothing else
        assert torch.equal(st.cpu(), (i.dt * i.x)[..., None] * i.Bm[:, None, :])


# -------------------------------------------------------- conv_update vs float64
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("shape", S.CONV_SHAPES, ids=SHAPE_ID)
def test_conv_update_vs_float64(shape, io):
    """bias / silu on and off; x and out row-strided views (as xz[:, :D] is),
    sentinels around out; the window bit for bit the fp32 inputs, oldest first."""
    B, D = shape
    worst = 0.0
    for o in S.CONV_OPTIONS:
        i = S.conv_inputs(B, D, io, o["bias"], o["silu"])
        d = _dev(i)
        xbuf = torch.full((B, 2 * D + 3), SENTINEL, device=DEV, dtype=io)
        xbuf[:, 1:1 + D] = d.x
        obuf = torch.full((B + 2, D + 7), SENTINEL, device=DEV, dtype=io)
        obuf0 = obuf.clone()
        out, st = _conv_update(d, x=xbuf[:, 1:1 + D], out=obuf[:B, 3:3 + D])
        worst = max(worst, S.check_conv(out, st, S.conv_reference(i), io, f"{shape} {S.opt_name(o)}"))
        obuf0[:B, 3:3 + D] = out
        assert torch.equal(obuf, obuf0), "an out store landed outside its view"
        out2, st2 = _conv_update(d)
        assert torch.equal(out, out2) and torch.equal(st, st2)
    _report(f"conv {shape}", io, io, {"out": worst})


# ------------------------------------------------------ prefill -> step hand-off
def test_prefill_to_step_handoff():
    """bf16, B = 3, D = 64: conv_fwd / scan_fwd on a ragged prompt (lengths 5,
    1, 0) hand their window and state to 6 steps of conv_update +
    state_update; compared with the float64 oracle on each row's own
    concatenated sequence.  Seven to eleven steps compound, with a bf16 u
    between conv and scan: close() at the bf16 tolerance of this file family
    (1e-2 of the maximum), not the per-element bound."""
    from mtts import ops
    B, D, L, T, N = 3, 64, 5, 6, S.N
    lens = [5, 1, 0]
    g = torch.Generator().manual_seed(561)
    rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
    bf = lambda t: t.to(BF16)                              # noqa: E731
    x, dl, z = bf(rn(B, L + T, D)), bf(0.5 * rn(B, L + T, D)), bf(rn(B, L + T, D))
    Bm, Cm = bf(rn(B, L + T, N)), bf(rn(B, L + T, N))
    w, cb = 0.5 * rn(D, 4), rn(D)
    A, Dp, bias = -(0.5 + 3.5 * torch.rand(D, N, generator=g)), rn(D), 0.1 * rn(D)
    # row b's sequence: its prompt x[b, :len_b], then the T steps x[b, L:]
    ys, lasts = [], []
    for b, n in enumerate(lens):
        seq = lambda t: torch.cat([t[b, :n], t[b, L:]]).double().t()[None]      # noqa: E731  (1, C, n + T)
        u, _ = R.causal_conv1d_ref(seq(x), w.double(), cb.double(), "silu")
        y, last = R.selective_scan_ref(u, seq(dl), A.double(), seq(Bm), seq(Cm), Dp.double(), seq(z), bias.double(),
                                       True, return_last_state=True)
        ys.append(y[0, :, n:].t())
        lasts.append(last[0])
    to = lambda t: t.to(DEV)                               # noqa: E731
    x, dl, z, Bm, Cm, w, cb, A, Dp, bias = map(to, (x, dl, z, Bm, Cm, w, cb, A, Dp, bias))
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    u, conv_state = ops.conv_fwd(x[:, :L], w, cb, True, want_state=True, seq_lens=sl)
    _, ssm_state, _ = ops.scan_fwd(u, dl[:, :L], A, Bm[:, :L], Cm[:, :L], Dp, z[:, :L], bias, True, want_last=True,
                                   seq_lens=sl)
    outs = []
    for t in range(L, L + T):
        ut = ops.conv_update(x[:, t], conv_state, w, cb, True)
        outs.append(ops.state_update(ssm_state, ut, dl[:, t], A, Bm[:, t], Cm[:, t], Dp, z[:, t], bias, True))
    close(torch.stack(outs, 1).float(), torch.stack(ys), rtol=1e-2, name="step outputs")
    close(ssm_state, torch.stack(lasts), rtol=1e-2, name="final state")
    want = torch.stack([torch.cat([x[b, :n], x[b, L:]])[-4:].t() for b, n in enumerate(lens)]).float()
    assert torch.equal(conv_state, want), "final conv window"


# ------------------------------------------------------------- front-end misuse
def _strided(t):
    """The same values with element stride 2."""
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=t.device, dtype=t.dtype)
    buf[..., ::2] = t
    return buf[..., ::2]


def _transposed(t):
    """The same values, the last two dimensions laid out the other way round."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


STATE_MISUSE = {
    "Cm:dtype": lambda d: dict(Cm=d.Cm.float()),
    "Bm:stride": lambda d: dict(Bm=_strided(d.Bm)),
    "dt:dtype": lambda d: dict(dt=d.dt.float()),
    "dt:stride": lambda d: dict(dt=_strided(d.dt)),
    "x:stride": lambda d: dict(x=_strided(d.x)),
    "z:dtype": lambda d: dict(z=d.z.float()),
    "z:stride": lambda d: dict(z=_strided(d.z)),
    "out:stride": lambda d: dict(out=_strided(torch.zeros_like(d.x))),
    "out:dtype": lambda d: dict(out=torch.zeros_like(d.x, dtype=F32)),
    "state:dtype": lambda d: dict(state=d.state.double()),
    "state:noncontiguous": lambda d: dict(state=_transposed(d.state)),
    "A:dtype": lambda d: dict(A=d.A.double()),
    "A:noncontiguous": lambda d: dict(A=_transposed(d.A)),
    "D:dtype": lambda d: dict(D=d.D.bfloat16()),
    "D:stride": lambda d: dict(D=_strided(d.D)),
    "dt_bias:dtype": lambda d: dict(dt_bias=d.dt_bias.bfloat16()),
    "dt_bias:stride": lambda d: dict(dt_bias=_strided(d.dt_bias)),
}
CONV_MISUSE = {
    "w:dtype": lambda d: dict(w=d.w.bfloat16()),
    "w:noncontiguous": lambda d: dict(w=_transposed(d.w)),
    "bias:dtype": lambda d: dict(bias=d.bias.bfloat16()),
    "bias:stride": lambda d: dict(bias=_strided(d.bias)),
    "conv_state:dtype": lambda d: dict(conv_state=d.conv_state.double()),
    "conv_state:noncontiguous": lambda d: dict(conv_state=_transposed(d.conv_state)),
    "x:stride": lambda d: dict(x=_strided(d.x)),
    "out:dtype": lambda d: dict(out=torch.zeros_like(d.x, dtype=F32)),
    "out:stride": lambda d: dict(out=_strided(torch.zeros_like(d.x))),
}
MISUSE = [("state_update", k) for k in STATE_MISUSE] + [("conv_update", k) for k in CONV_MISUSE]


@pytest.mark.parametrize("op,case", MISUSE, ids=[f"{o}-{c}" for o, c in MISUSE])
def test_front_end_never_returns_wrong_numbers(op, case):
    """One argument of another dtype or layout than the kernel reads (bf16
    I/O, so that every fp32 argument has a dtype to be confused with): the
    front end converts it and the result meets the float64 bound, or it raises
    TypeError / ValueError naming the argument and leaves the state alone."""
    arg = case.split(":")[0]
    if op == "state_update":
        i = S.state_inputs(5, 96, BF16, BF16)
        d = _dev(i)
        over = STATE_MISUSE[case](d)
        state, out = over.pop("state", d.state.clone()), over.pop("out", None)
        run = lambda: _state_update(d, state=state, out=out, **over)                              # noqa: E731
        judge = lambda y, st: S.check_state(y, st, S.state_reference(i), BF16, case)              # noqa: E731
    else:
        i = S.conv_inputs(5, 96, BF16)
        d = _dev(i)
        over = CONV_MISUSE[case](d)
        state, out = over.pop("conv_state", d.conv_state.clone()), over.pop("out", None)
        run = lambda: _conv_update(d, state=state, out=out, **over)                               # noqa: E731
        judge = lambda y, st: S.check_conv(y, st, S.conv_reference(i), BF16, case)                # noqa: E731
    before = state.clone()
    try:
        y, st = run()
    except (TypeError, ValueError) as e:
        assert f"{op}: {arg} " in str(e), f"{case}: the error does not name {arg}: {e}"
        assert torch.equal(state, before), f"{case}: raised after touching the state"
        print(f"MISUSE {op} {case}: raises {type(e).__name__}: {e}")
    else:
        assert st.data_ptr() == state.data_ptr()
        judge(y, st.contiguous())
        print(f"MISUSE {op} {case}: converts")
