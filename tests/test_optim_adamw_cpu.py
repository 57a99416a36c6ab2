"""CPU side of FusedClipAdamW (mtts/optim.py, csrc/optim.hip mtts_clip_adamw):
the float32 restatement of the kernel (optim_adamw_ref.Restated) held to the
float64 twin (GroupTwin) by the project's criterion, test_optim_ref_cpu.
update_close (max|dp - dp_ref| <= 1e-2 * max|dp_ref| per tensor), the mutants
it must reject, the schedule's values, the host's ValueErrors and the ABI.

Setup: shapes (70000,), (7,), (300, 5) in three groups (clipped decoupled wd
0.01; clipped wd 0; unclipped L2 wd 0.01 at twice the lr), beta (0.9, 0.95),
clip 1.0, six steps, gradients alternating scale 0.01 and 3.

Measured update error / max|dp_ref| of the right restatement: lr 1e-2 constant
<= 4.6e-5, cosine (W = 3, T = 8, r = 0.1) <= 1.6e-4; lr 1e-4 constant 2.7e-3 to
4.2e-3.  The last is the thin case: p * (1 - lr wd) and the subtraction each
round p (half-ulp 2.4e-7 at |p| in [4, 8)) against an update of 1e-4, up to
4.8e-3, so the margin under the 1e-2 bound is about 2.4x.  A schedule factor
f < 1 at lr 1e-4 shrinks the update below that rounding (f = 1/3: up to 1.4e-2
for a right kernel), so the schedule is exercised at lr 1e-2.  Mutants: decay
as L2 1.9 to 2.0; schedule one step off 8.6e-2 (t = 3) to 1.0; norm over all
groups 0.84 to 0.96 from the step that tells it apart; a skipped step that
advances the counter 0.18.  EMA (lr 1e-2, decay 0.9): per-step delta error
5.8e-5 to 7.8e-4 for the right restatement, 0.16 to 1.0 for the EMA taken from
the old parameter."""
import ctypes
import functools
import math
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT
from optim_adamw_ref import CONSTANT, KINDS, GroupTwin, Restated, sched_factor
from test_optim_ref_cpu import UPDATE_RTOL, off_singular_point, rel_err, update_close, update_err

from mtts.optim import FusedClipAdamW, LRSchedule

BETAS, EPS, STEPS = (0.9, 0.95), 1e-8, 6
COSINE = ("cosine", 3, 8, 0.1)


def make_groups(lr, seed=0, spike=False):
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=gen) for s in [(70000,), (7,), (300, 5)]]
    groups = [dict(init=[init[0]], lr=lr, wd=0.01, decoupled=True, clip=True),
              dict(init=[init[1]], lr=lr, wd=0.0, decoupled=True, clip=True),
              dict(init=[init[2]], lr=2 * lr, wd=0.01, decoupled=False, clip=False)]
    grads = []
    for k in range(STEPS):
        gs = [[torch.randn(t.shape, generator=gen) * (3.0 if k % 2 else 0.01) for t in g["init"]] for g in groups]
        if k == 0:      # the L2 group's first step off the point where g + wd p cancels (test_optim_ref_cpu)
            gs[2] = off_singular_point(groups[2]["init"], gs[2], 0.01, None)[0]
        if spike and k == 3:     # the unclipped group alone, 100x: moves only a norm that wrongly counts it
            gs[2] = [g * 100.0 for g in gs[2]]
        grads.append(gs)
    return groups, grads


@functools.lru_cache(maxsize=None)
def run(lr, sched=CONSTANT, ema_decay=None, mutant=None, spike=False):
    """STEPS steps of the restatement (or a mutant) beside the twin; per step
    the worst update / EMA-delta error over the tensors, and moment, norm, lr errors."""
    groups, grads = make_groups(lr, spike=spike)
    k = Restated(groups, BETAS, EPS, 1.0, sched, ema_decay, mutant=mutant)
    twin = GroupTwin(groups, BETAS, EPS, 1.0, sched, ema_decay)
    rows = []
    for step in range(STEPS):
        before = [[p.clone() for p in ps] for ps in k.ps]
        e_before = [[e.clone() for e in es] for es in k.es]
        k.step(grads[step])
        ref_before, ref_e_before, total = twin.step(grads[step])
        row = {"update": 0.0, "ema": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
        for gi in range(len(groups)):
            for i in range(len(groups[gi]["init"])):
                err, scale = update_err(before[gi][i], k.ps[gi][i], ref_before[gi][i], twin.values()[gi][i])
                row["update"] = max(row["update"], err / scale)
                if ema_decay is not None:
                    err, scale = update_err(e_before[gi][i], k.es[gi][i], ref_e_before[gi][i], twin.ema[gi][i])
                    row["ema"] = max(row["ema"], err / scale)
                rm, rv = twin.moments(gi, i)
                row["exp_avg"] = max(row["exp_avg"], rel_err(k.ms[gi][i], rm))
                row["exp_avg_sq"] = max(row["exp_avg_sq"], rel_err(k.vs[gi][i], rv))
        row["norm"] = rel_err(k.norm, total)
        row["lr"] = max(abs(float(a) - b) / b for a, b in zip(k.lr, twin.lr))
        rows.append(row)
    return rows


def show(tag, rows, key="update"):
    print(f"{tag}: " + " ".join(f"{r[key]:.2e}" for r in rows))


@pytest.mark.parametrize("lr,sched", [(1e-2, CONSTANT), (1e-2, COSINE), (1e-4, CONSTANT)])
def test_restatement_passes_update_criterion(lr, sched):
    rows = run(lr, sched)
    show(f"lr={lr} {sched[0]}", rows)
    for k, r in enumerate(rows):
        assert r["update"] <= UPDATE_RTOL, f"step {k + 1}: update error {r['update']:.3e}"
        assert r["exp_avg"] <= 1e-5 and r["exp_avg_sq"] <= 1e-5 and r["norm"] <= 1e-5 and r["lr"] <= 1e-6, (k, r)


def test_restatement_passes_ema_criterion():
    rows = run(1e-2, COSINE, ema_decay=0.9)
    show("ema", rows, "ema")
    assert all(r["ema"] <= UPDATE_RTOL and r["update"] <= UPDATE_RTOL for r in rows)


@pytest.mark.parametrize("lr", [1e-2, 1e-4])
def test_decay_applied_as_l2_fails(lr):
    """AdamW's p *= 1 - lr wd replaced by Adam's g += wd p in the decoupled
    group: at the 0.01-scale steps the clipped gradient no longer dominates."""
    rows = run(lr, mutant="l2_decay")
    show(f"l2 lr={lr}", rows)
    assert max(r["update"] for r in rows) > 10 * UPDATE_RTOL
    assert sum(r["update"] > UPDATE_RTOL for r in rows) >= 3


def test_schedule_one_step_off_fails():
    rows = run(1e-2, COSINE, mutant="sched_off")
    show("sched_off", rows)
    # f(t + 1) / f(t) = 2, 1.5 in the warm-up, then the cosine's slope (0.914 at t = 3)
    assert all(r["update"] > 3 * UPDATE_RTOL for r in rows)
    assert rows[0]["lr"] > 0.5


def test_ema_from_the_old_parameter_fails():
    rows = run(1e-2, COSINE, ema_decay=0.9, mutant="ema_old_p")
    show("ema_old_p", rows, "ema")
    assert all(r["update"] <= UPDATE_RTOL for r in rows)        # the parameters are right
    assert all(r["ema"] > 10 * UPDATE_RTOL for r in rows)
    assert rows[0]["ema"] == 1.0                                 # e = p_old at the first step: no delta at all


@pytest.mark.parametrize("lr", [1e-2, 1e-4])
def test_norm_over_all_groups_fails(lr):
    """The unclipped group's gradients counted into the clip norm.  The norm
    misses its 1e-5 bound at every step (the group is 2 % of the elements).
    Adam's update barely feels a clip coefficient that is off by the same
    factor at every step, so the unclipped group's gradients are 100x larger
    at the fourth step alone: the clipped groups' update misses its bound there
    under the mutant, and the right restatement passes at every step."""
    rows = run(lr, spike=True)
    show(f"right, spike lr={lr}", rows)
    assert all(r["update"] <= UPDATE_RTOL and r["norm"] <= 1e-5 for r in rows)
    rows = run(lr, mutant="norm_all", spike=True)
    show(f"norm_all lr={lr}", rows)
    assert all(r["norm"] > 1e-3 for r in rows)
    assert rows[3]["update"] > 10 * UPDATE_RTOL


def skip_run(mutant, bad_group):
    """Three good steps with an inf gradient step after the second; the twin
    never sees the bad step."""
    groups, grads = make_groups(1e-2)
    k = Restated(groups, BETAS, EPS, 1.0, COSINE, 0.9, skip_nonfinite=True, mutant=mutant)
    twin = GroupTwin(groups, BETAS, EPS, 1.0, COSINE, 0.9)
    for step in range(2):
        k.step(grads[step])
        twin.step(grads[step])
    bad = [[g.clone() for g in gs] for gs in grads[2]]
    bad[bad_group][0].view(-1)[3] = float("inf")
    snap = [[t.clone() for t in ts] for ts in k.ps + k.ms + k.vs + k.es]
    k.step(bad)
    assert k.skipped == 1
    assert all(torch.equal(a, b) for ts, ss in zip(k.ps + k.ms + k.vs + k.es, snap) for a, b in zip(ts, ss))
    steps_after_skip = list(k.gsteps)
    before = [[p.clone() for p in ps] for ps in k.ps]
    k.step(grads[2])
    ref_before, _, _ = twin.step(grads[2])
    return steps_after_skip, [update_err(before[gi][0], k.ps[gi][0], ref_before[gi][0], twin.values()[gi][0])
                              for gi in range(3)]


@pytest.mark.parametrize("bad_group", [0, 2], ids=["clipped", "unclipped"])
def test_skipped_step_leaves_the_counters(bad_group):
    steps, errs = skip_run(None, bad_group)
    assert steps == [2, 2, 2]
    assert all(err <= UPDATE_RTOL * scale for err, scale in errs)
    steps, errs = skip_run("skip_advances", bad_group)
    assert steps == [3, 3, 3]
    print("skip_advances:", " ".join(f"{e / s:.2e}" for e, s in errs))
    assert all(err > UPDATE_RTOL * scale for err, scale in errs)     # bias corrections and schedule one step ahead


def test_update_close_rejects_a_mutant_step():
    groups, grads = make_groups(1e-2)
    k, twin = Restated(groups, BETAS, EPS, 1.0, mutant="l2_decay"), GroupTwin(groups, BETAS, EPS, 1.0)
    for step in range(2):
        before = k.ps[0][0].clone()
        k.step(grads[step])
        ref_before, _, _ = twin.step(grads[step])
    with pytest.raises(AssertionError):
        update_close(before, k.ps[0][0], ref_before[0][0], twin.values()[0][0])


# ------------------------------------------------------------------ schedule
W3 = {  # kind -> f(t) at W = 3, T = 8, r = 0.1 for t = 1, 2, 3, 4, 8, 13, written out
    "constant": [1 / 3, 2 / 3, 1.0, 1.0, 1.0, 1.0],
    "cosine": [1 / 3, 2 / 3, 1.0, 0.1 + 0.45 * (1 + math.cos(0.2 * math.pi)), 0.1, 0.1],
    "linear": [1 / 3, 2 / 3, 1.0, 0.1 + 0.9 * 0.8, 0.1, 0.1],
    "inverse_sqrt": [1 / 3, 2 / 3, 1.0, math.sqrt(3 / 4), math.sqrt(3 / 8), math.sqrt(3 / 13)],
}
W0 = {  # W = 0, T = 8, r = 0.1
    "constant": [1.0] * 6,
    "cosine": [0.1 + 0.45 * (1 + math.cos(math.pi * t / 8)) for t in (1, 2, 3, 4)] + [0.1, 0.1],
    "linear": [0.1 + 0.9 * (1 - t / 8) for t in (1, 2, 3, 4)] + [0.1, 0.1],
    "inverse_sqrt": [1.0, math.sqrt(1 / 2), math.sqrt(1 / 3), 0.5, math.sqrt(1 / 8), math.sqrt(1 / 13)],
}
TS = (1, 2, 3, 4, 8, 13)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,table", [(3, W3), (0, W0)], ids=["W3", "W0"])
def test_schedule_values(kind, W, table):
    host = LRSchedule(kind, warmup_steps=W, total_steps=8, min_ratio=0.1)
    for t, want in zip(TS, table[kind]):
        assert sched_factor(kind, W, 8, 0.1, t) == pytest.approx(want, rel=1e-15, abs=1e-16), (kind, t)
        assert host.factor(t) == sched_factor(kind, W, 8, 0.1, t)


def test_inverse_sqrt_floor():
    assert sched_factor("inverse_sqrt", 3, 0, 0.6, 13) == 0.6 and LRSchedule("inverse_sqrt", 3, 0, 0.6).factor(13) == 0.6


# --------------------------------------------------------------- host errors
def P(*shape):
    return torch.nn.Parameter(torch.zeros(*shape))


def test_value_errors_before_anything_is_allocated():
    with pytest.raises(ValueError, match="at most 64"):
        FusedClipAdamW([{"params": [P(2)]} for _ in range(65)])
    FusedClipAdamW([{"params": [P(2)]} for _ in range(64)])
    with pytest.raises(ValueError, match="per optimizer"):
        FusedClipAdamW([{"params": [P(2)]}, {"params": [P(2)], "betas": (0.8, 0.999)}])
    with pytest.raises(ValueError, match="per optimizer"):
        FusedClipAdamW([{"params": [P(2)]}, {"params": [P(2)], "eps": 1e-6}])
    for kind in ("cosine", "linear"):
        for T in (3, 2):
            with pytest.raises(ValueError, match="total_steps > warmup_steps"):
                FusedClipAdamW([P(2)], schedule=dict(kind=kind, warmup_steps=3, total_steps=T))
    FusedClipAdamW([P(2)], schedule=dict(kind="constant", warmup_steps=3))
    FusedClipAdamW([P(2)], schedule=dict(kind="inverse_sqrt", warmup_steps=3))
    for r in (-0.1, 1.1):
        with pytest.raises(ValueError, match="min_ratio"):
            FusedClipAdamW([P(2)], schedule=dict(kind="cosine", warmup_steps=3, total_steps=8, min_ratio=r))
    for d in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedClipAdamW([P(2)], ema_decay=d)
    FusedClipAdamW([P(2)], ema_decay=0.0)
    with pytest.raises(ValueError, match="fp32"):
        FusedClipAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match="dense"):
        FusedClipAdamW([torch.nn.Parameter(torch.zeros(4, 4).to_sparse())])
    with pytest.raises(ValueError, match="dense"):
        FusedClipAdamW([torch.nn.Parameter(torch.zeros(4, 4)[:, ::2])])
    with pytest.raises(ValueError, match="kind"):
        FusedClipAdamW([P(2)], schedule=dict(kind="step"))


def test_group_keys_and_defaults():
    opt = FusedClipAdamW([{"params": [P(2)], "clip": False, "lr": 3e-4}, {"params": [P(3)], "decoupled": False}],
                         lr=1e-3, weight_decay=0.1)
    a, b = opt.param_groups
    assert (a["lr"], a["weight_decay"], a["decoupled"], a["clip"]) == (3e-4, 0.1, True, False)
    assert (b["lr"], b["weight_decay"], b["decoupled"], b["clip"]) == (1e-3, 0.1, False, True)
    assert opt.last_grad_norm is None and opt.skipped_steps is None and opt._dev is None
    assert opt.step() is None                 # no gradients: nothing to launch, nothing allocated
    assert opt._dev is None
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_parameters()
    # a torch.optim.AdamW state_dict loads: the group keys it lacks take the defaults
    ref = torch.optim.AdamW([P(2), P(3)], lr=1e-3)
    one = FusedClipAdamW([P(2), P(3)], lr=1e-3, decoupled=False)
    one.load_state_dict(ref.state_dict())
    assert one.param_groups[0]["decoupled"] is False and one.param_groups[0]["clip"] is True
    ref.load_state_dict(one.state_dict())


# ------------------------------------------------------------------------ ABI
STRUCTS = {"MttsAdamWTensor": "AdamWTensor", "MttsAdamWGroup": "AdamWGroup", "MttsLrSchedule": "LrSchedule",
           "MttsAdamWArgs": "AdamWArgs"}
CONSTS = {"MTTS_ADAMW_MAX_GROUPS": "ADAMW_MAX_GROUPS", "MTTS_ADAMW_OUT_LR": "ADAMW_OUT_LR",
          "MTTS_ADAMW_OUT_STEP": "ADAMW_OUT_STEP", "MTTS_ADAMW_OUT_BC2": "ADAMW_OUT_BC2",
          "MTTS_ADAMW_OUT_DECAY": "ADAMW_OUT_DECAY", "MTTS_ADAMW_OUT_FLOATS": "ADAMW_OUT_FLOATS"}
C_KINDS = {"MTTS_LR_CONSTANT": "constant", "MTTS_LR_COSINE": "cosine", "MTTS_LR_LINEAR": "linear",
           "MTTS_LR_INV_SQRT": "inverse_sqrt"}


def test_adamw_structs_match_the_header():
    from mtts import _lib
    header = os.path.join(ROOT, "include", "mtts.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'printf("{pyname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    for cname in list(CONSTS) + list(C_KINDS):
        lines.append(f'printf("const {cname} %d\\n", (int){cname});')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        py, field, val = line.split()
        if py == "const":
            got = getattr(_lib, CONSTS[field]) if field in CONSTS else _lib.LR_KINDS[C_KINDS[field]]
        else:
            cls = getattr(_lib, py)
            got = ctypes.sizeof(cls) if field == "size" else getattr(cls, field).offset
        assert got == int(val), f"{py}.{field}: ctypes {got} != C {val}"
        seen += 1
    assert seen == sum(1 + len(getattr(_lib, p)._fields_) for p in STRUCTS.values()) + len(CONSTS) + len(C_KINDS)
    assert ctypes.sizeof(_lib.AdamWGroup) == 16 and ctypes.sizeof(_lib.AdamWTensor) == 64


def test_adamw_symbol_is_exported():
    from mtts import _lib
    lib = _lib.lib()
    assert hasattr(lib, "mtts_clip_adamw") and "mtts_clip_adamw" in _lib.exported_symbols()
    assert lib.mtts_abi_version() == 15
