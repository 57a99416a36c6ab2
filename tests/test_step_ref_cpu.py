"""tests/step_ref.py proven on the CPU: the single-step float64 references
against the sequence oracle over 12 steps, the float32 evaluation of the same
formulas against the criterion on every case list tests/test_gpu_step.py runs
(the bound can be met, at the K the GPU file uses), and the criterion against
the mutants it has to tell from a right kernel.

Measured here, err / (eps cond) of the float32 evaluation: state <= 2.3 and
y <= 2.8 over the option / dtype / shape grid, <= 2.3 and 2.5 over the fused
ranks, <= 2.0 at the edges, conv <= 2.8; K is 16.  The mutants: a dropped
state 4e4 and more in y; the window shifted 7e5 and more; log(1 + e) in place
of log1p(e) 60 and 109 in the state of the two shapes it is run on, where
softplus(dt_bias) is 1e-3 to 1e-1 as under a trained layer's bias."""
import pytest
import torch

import step_ref as S
from oracle import mamba_ref as R

F32, BF16, F64 = S.F32, S.BF16, S.F64
PAIRS = [pytest.param(io, bc, id=f"{S.TAG[io]}-{S.TAG[bc]}") for io, bc in S.DTYPE_PAIRS]
IOS = [pytest.param(io, id=S.TAG[io]) for io in (F32, BF16)]


def _opts(o):
    return dict(has_D=o["D"], has_z=o["z"], has_bias=o["bias"], softplus=o["softplus"])


def test_state_reference_is_the_scan_oracle_over_12_steps():
    B, D, L = 3, 7, 12
    base = S.state_inputs(B, D)
    g = torch.Generator().manual_seed(12)
    u, dl, z = (torch.randn(B, D, L, generator=g, dtype=F64) for _ in range(3))
    Bm, Cm = (torch.randn(B, S.N, L, generator=g, dtype=F64) for _ in range(2))
    h0 = base.state.double()
    ref, last = R.selective_scan_ref(u, dl, base.A.double(), Bm, Cm, base.D.double(), z, base.dt_bias.double(), True,
                                     h0=h0, return_last_state=True)
    h = h0
    for t in range(L):
        i = S.types.SimpleNamespace(io=F32, bc=F32, softplus=True, rank=0, dt_w=None, state=h, x=u[..., t],
                                    dt=dl[..., t], A=base.A, Bm=Bm[..., t], Cm=Cm[..., t], D=base.D, z=z[..., t],
                                    dt_bias=base.dt_bias)
        r = S.state_reference(i)
        assert (r["y"] - ref[..., t]).abs().max() <= 1e-12 * ref.abs().max()
        assert (r["cond_h"] >= r["state"].abs() * (1 - 1e-12)).all() and (r["cond_y"] >= 0).all()
        h = r["state"]
    assert (h - last).abs().max() <= 1e-12 * last.abs().max()


def test_fused_reference_is_the_unfused_one_on_the_float64_product():
    i = S.state_inputs(*S.FUSED_SHAPE, BF16, BF16, rank=7)
    r = S.state_reference(i)
    j = S.types.SimpleNamespace(**vars(i))
    j.dt, j.dt_w = i.dt.double() @ i.dt_w.double().t(), None
    q = S.state_reference(j)
    assert torch.equal(r["y"], q["y"]) and torch.equal(r["state"], q["state"])
    assert (r["cond_h"] >= q["cond_h"]).all()          # the dot's own allowance comes on top


@pytest.mark.parametrize("silu", [True, False])
def test_conv_reference_is_the_conv_oracle_over_12_steps(silu):
    B, D, L = 3, 7, 12
    base = S.conv_inputs(B, D, F32, True, silu)
    g = torch.Generator().manual_seed(13)
    xs = torch.randn(B, D, L, generator=g, dtype=F64)
    act = "silu" if silu else None
    ref, last = R.causal_conv1d_ref(xs, base.w.double(), base.bias.double(), act, conv_state=base.conv_state.double())
    st = base.conv_state.double()
    for t in range(L):
        i = S.types.SimpleNamespace(io=F32, silu=silu, x=xs[..., t], conv_state=st, w=base.w, bias=base.bias)
        r = S.conv_reference(i)
        assert (r["out"] - ref[..., t]).abs().max() <= 1e-12 * ref.abs().max()
        assert (r["cond"] >= r["out"].abs() * (1 - 1e-12)).all()
        st = r["conv_state"]
    assert torch.equal(st, last)


# ------------------------------------------------------------ the bound can be met
@pytest.mark.parametrize("io,bc", PAIRS)
@pytest.mark.parametrize("shape", S.STATE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_state_update_meets_the_bound(shape, io, bc):
    worst = {"y": 0.0, "state": 0.0}
    for o in S.OPTIONS:
        i = S.state_inputs(*shape, io, bc, **_opts(o))
        y, st = S.state_float32(i)
        q = S.check_state(y, st, S.state_reference(i), io, S.opt_name(o))
        worst = {k: max(worst[k], q[k]) for k in q}
    print(shape, S.TAG[io], S.TAG[bc], worst)


@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("rank", S.FUSED_RANKS)
def test_float32_fused_dt_proj_meets_the_bound(rank, io):
    i = S.state_inputs(*S.FUSED_SHAPE, io, io, rank=rank)
    y, st = S.state_float32(i)
    print(rank, S.TAG[io], S.check_state(y, st, S.state_reference(i), io))


@pytest.mark.parametrize("edge", S.EDGES)
def test_float32_edge_values_meet_the_bound(edge):
    i = S.edge_inputs(edge)
    y, st = S.state_float32(i)
    print(edge, S.check_state(y, st, S.state_reference(i), F32))
    if edge == "exp_underflow":
        assert torch.equal(st, (i.dt * i.x)[..., None] * i.Bm[:, None, :])


@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("shape", S.CONV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_conv_update_meets_the_bound(shape, io):
    for o in S.CONV_OPTIONS:
        i = S.conv_inputs(*shape, io, o["bias"], o["silu"])
        out, st = S.conv_float32(i)
        print(shape, S.TAG[io], o, S.check_conv(out, st, S.conv_reference(i), io, S.opt_name(o)))


# ------------------------------------------------------------- and tells a wrong kernel
@pytest.mark.parametrize("io,bc", PAIRS)
@pytest.mark.parametrize("shape", S.STATE_SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dropped_state_misses_the_bound(shape, io, bc):
    """y without the 16th state: caught on every dtype pair and every shape of
    more than one element (a single bf16 y can hide one term of 16 in its own
    rounding), with every option on and with every option off."""
    for o in (S.OPTIONS[0], S.OPTIONS[-1]):
        i = S.state_inputs(*shape, io, bc, **_opts(o))
        ref = S.state_reference(i)
        y, st = S.state_float32(i, "dropped_state")
        q = S.state_ratios(y, st, ref)
        print(shape, S.opt_name(o), q)
        assert q["state"] <= S.K             # the state is right,
        with pytest.raises(AssertionError):  # y is not
            S.check_state(y, st, ref, io)
        S.check_state(*S.state_float32(i), ref, io)


@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("shape", S.CONV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shifted_window_misses_the_bound(shape, io):
    for o in S.CONV_OPTIONS:
        i = S.conv_inputs(*shape, io, o["bias"], o["silu"])
        ref = S.conv_reference(i)
        out, st = S.conv_float32(i, "window_shifted")
        print(shape, o, S.ratio(out, ref["out"], ref["cond"]))
        with pytest.raises(AssertionError):
            S.check_conv(out, st, ref, io)
    # and a window that is right in value but one slot late is caught by the bit-exact comparison
    good, st = S.conv_float32(i)
    with pytest.raises(AssertionError):
        S.check_conv(good, torch.roll(st, 1, -1), ref, io)


@pytest.mark.parametrize("shape", [(5, 96), (33, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_softplus_with_a_rounded_sum_misses_the_bound(shape):
    """log(1 + e^p) with the sum rounded to fp32 is eps accurate absolutely,
    not relatively: under a trained layer's bias (softplus(bias) 1e-3 to 1e-1)
    the step, and through it the state, is off by hundreds of eps cond.  This
    is the form csrc/step.hip used before this suite."""
    i = S.state_inputs(*shape, F32, F32)
    ref = S.state_reference(i)
    y, st = S.state_float32(i, "softplus_log_1_plus")
    q = S.state_ratios(y, st, ref)
    print(shape, q)
    assert q["state"] > S.K
    with pytest.raises(AssertionError):
        S.check_state(y, st, ref, F32)


def test_ratio_rejects_nan_a_wrong_dtype_and_more_than_one_bf16_rounding():
    i = S.state_inputs(5, 96, BF16, BF16)
    ref = S.state_reference(i)
    y, st = S.state_float32(i)
    bad = st.clone()
    bad[2, 3, 4] = float("nan")
    assert S.ratio(bad, ref["state"], ref["cond_h"]) == float("inf")
    with pytest.raises(AssertionError):
        S.check_state(y.float(), st, ref, BF16)
    k = ref["y"].abs().argmax()
    y2 = y.clone()
    y2.view(-1)[k] = (ref["y"].view(-1)[k] * (1 + 3 * S.BF16_ULP)).bfloat16()
    with pytest.raises(AssertionError):
        S.check_state(y2, st, ref, BF16)
    # cond = 0 (x = 0 on a zero state): only the exact result passes
    j = S.types.SimpleNamespace(**vars(S.edge_inputs("x_zero")))
    j.state = torch.zeros_like(j.state)
    r = S.state_reference(j)
    assert (r["cond_h"] == 0).all()
    assert S.ratio(torch.zeros_like(j.state), r["state"], r["cond_h"]) == 0.0
    assert S.ratio(torch.full_like(j.state, 1e-30), r["state"], r["cond_h"]) == float("inf")


def test_case_lists_are_the_ones_the_suite_promises():
    assert len(S.OPTIONS) == 16 and len({S.opt_name(o) for o in S.OPTIONS}) == 16
    assert S.OPTIONS[0] == dict(D=True, z=True, bias=True, softplus=True) and not any(S.OPTIONS[-1].values())
    assert (3, 80) in S.STATE_SHAPES and 3 * 80 * 4 % 256 != 0         # tail quads in the last block
    assert any(r % 32 == 0 for r in S.FUSED_RANKS) and any(r % 8 in (1, 2, 3, 4) for r in S.FUSED_RANKS)
    assert len(S.EDGES) == 12
