"""GPU parity of FusedClipAdamW (mtts_clip_adamw) against the float64 twin of
optim_adamw_ref (clip_grad_norm_ over the clipped groups, torch.optim.AdamW /
Adam per group, the schedule restated in Python, EMA in float64), its
bit-equality with FusedClipAdam where the two compute the same thing, and the
non-finite guard.

Bounds: the update and the EMA's per-step delta by test_optim_ref_cpu.
update_close (1e-2 of the tensor's largest reference delta); norm over the
clipped set and the moments 1e-5; last_lr 1e-6 (a double cast once to fp32 is
6e-8; the rest is room for the device's cos).  EMA is held to its criterion
only in the run at lr = 1e-2, decay = 0.9, where its delta (~1e-3) stands clear
of fp32's rounding of the average (test_optim_adamw_cpu's docstring).
The measured errors go to the file MTTS_OPTIM_ADAMW_PARITY names
(profiles/optim_adamw_parity.txt)."""
import os

import pytest
import torch

from optim_adamw_ref import CONSTANT, GroupTwin, record_adamw, write_adamw_parity
from test_gpu_ops import close, DEV
from test_optim_ref_cpu import off_singular_point, rel_err, update_close

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.95), 1e-8
CHUNK = 65536
COSINE = ("cosine", 3, 8, 0.1)
VIEW_N = 70


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    write_adamw_parity(os.environ.get("MTTS_OPTIM_ADAMW_PARITY"))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def offset_view(n, fill=0.0):
    """A view at a one-element storage offset: 4 bytes off 16-byte alignment."""
    buf = torch.full((n + 10,), fill, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[1:1 + n]


# group -> (shapes, lr multiple, wd, decoupled, clip); the last tensor of group 0 is the offset view, the last of
# group 1 never gets a gradient
SPEC = [([(CHUNK,), (CHUNK + 1,), (VIEW_N,)], 1.0, 0.01, True, True),
        ([(7,), (1,), (5,)], 1.0, 0.0, True, True),
        ([(33, 5)], 2.0, 0.01, False, False)]
NO_GRAD = (1, 2)


class Setup:
    def __init__(self, lr, sched=CONSTANT, ema_decay=None, max_norm=1.0, seed=0, **kw):
        from mtts.optim import FusedClipAdamW, LRSchedule
        self.gen = torch.Generator().manual_seed(seed)
        self.groups = [dict(init=[torch.randn(*s, generator=self.gen) for s in shapes], lr=lr * mult, wd=wd,
                            decoupled=dec, clip=clip) for shapes, mult, wd, dec, clip in SPEC]
        self.gp = [[torch.nn.Parameter(t.clone().to(DEV)) for t in g["init"]] for g in self.groups]
        view = offset_view(VIEW_N)
        view.copy_(self.groups[0]["init"][2])
        self.gp[0][2] = torch.nn.Parameter(view)
        self.gview = offset_view(VIEW_N, float("nan"))     # its gradient: a read past the view would poison the norm
        assert self.gp[0][2].data_ptr() % 16 == 4 and self.gview.data_ptr() % 16 == 4
        self.opt = FusedClipAdamW(
            [dict(params=ps, lr=g["lr"], weight_decay=g["wd"], decoupled=g["decoupled"], clip=g["clip"])
             for ps, g in zip(self.gp, self.groups)], lr=lr, betas=BETAS, eps=EPS, max_grad_norm=max_norm,
            schedule=LRSchedule(*sched), ema_decay=ema_decay, **kw)
        self.twin = GroupTwin(self.groups, BETAS, EPS, max_norm, sched, ema_decay)
        self.ema = ema_decay is not None
        self.static = False

    def draw(self, step, absent=()):
        """Gradients of one step (CPU): scale alternating 0.01 / 3, None for the
        tensor that never has one and for the groups in `absent`; the L2 group's
        first step is kept off the point where g + wd p cancels."""
        grads = [[torch.randn(t.shape, generator=self.gen) * (3.0 if step % 2 else 0.01) for t in g["init"]]
                 for g in self.groups]
        if step == 0:
            grads[2] = off_singular_point(self.groups[2]["init"], grads[2], 0.01, None)[0]
        grads[NO_GRAD[0]][NO_GRAD[1]] = None
        for gi in absent:
            grads[gi] = [None] * len(grads[gi])
        return grads

    def set_grads(self, grads):
        for gi, gs in enumerate(grads):
            for i, g in enumerate(gs):
                p = self.gp[gi][i]
                if g is None:
                    p.grad = None
                elif self.static and p.grad is not None:
                    p.grad.copy_(g)
                elif (gi, i) == (0, 2):
                    self.gview.copy_(g)
                    p.grad = self.gview
                else:
                    p.grad = g.to(DEV)

    def snapshot(self):
        ema = [[self.opt.state[p]["ema"].clone() if "ema" in self.opt.state.get(p, {}) else p.detach().clone()
                for p in ps] for ps in self.gp] if self.ema else None
        return [[p.detach().clone() for p in ps] for ps in self.gp], ema

    def check(self, name, grads, before, ema_before):
        """After one step of the optimizer on `grads`: step the twin and compare."""
        opt, twin = self.opt, self.twin
        ref_before, ref_ema_before, total = twin.step(grads)
        errs = {"update": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
        close(opt.last_grad_norm, total, rtol=1e-5, name=f"{name} norm")
        errs["norm"] = rel_err(opt.last_grad_norm, total)
        lrs = opt.last_lr.tolist()
        errs["last_lr"] = max(abs(a - b) / b for a, b in zip(lrs, twin.lr))
        print(f"{name}: last_lr {lrs} vs {twin.lr}")
        assert errs["last_lr"] <= 1e-6, f"{name}: last_lr {lrs} vs {twin.lr}"
        assert abs(float(opt.last_lr_factor) - twin.factor) <= 1e-6 * twin.factor
        for gi, gs in enumerate(grads):
            for i, g in enumerate(gs):
                p, tag = self.gp[gi][i], f"{name} g{gi} p{i}"
                if g is None:
                    assert torch.equal(bits(p), bits(before[gi][i])), f"{tag}: stepped without a gradient"
                    continue
                errs["update"] = max(errs["update"], update_close(before[gi][i], p, ref_before[gi][i],
                                                                  twin.values()[gi][i], name=tag))
                st, (rm, rv) = opt.state[p], twin.moments(gi, i)
                close(st["exp_avg"], rm, rtol=1e-5, name=f"{tag} m")
                close(st["exp_avg_sq"], rv, rtol=1e-5, name=f"{tag} v")
                errs["exp_avg"] = max(errs["exp_avg"], rel_err(st["exp_avg"], rm))
                errs["exp_avg_sq"] = max(errs["exp_avg_sq"], rel_err(st["exp_avg_sq"], rv))
                if self.ema:
                    errs["ema"] = max(errs.get("ema", 0.0), update_close(
                        ema_before[gi][i], st["ema"], ref_ema_before[gi][i], twin.ema[gi][i], name=f"{tag} ema"))
        print(f"{name}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        record_adamw(name, **errs)

    def step_and_check(self, name, step, absent=(), run=None):
        grads = self.draw(step, absent)
        self.set_grads(grads)
        before, ema_before = self.snapshot()
        gsnap = bits(self.gview._base)
        (run or self.opt.step)()
        assert torch.equal(bits(self.gview._base), gsnap), "gradient buffer rewritten"
        self.check(name, grads, before, ema_before)


@pytest.mark.parametrize("lr,sched,ema_decay", [(1e-2, COSINE, 0.9), (1e-4, CONSTANT, None)],
                         ids=["lr1e-2-cosine-ema", "lr1e-4-constant"])
def test_three_groups_vs_float64_twin(lr, sched, ema_decay):
    """Six steps of the three groups: clipped decoupled wd 0.01 (a full chunk,
    one element more, and the offset view: the scalar paths of both kernels),
    clipped wd 0 (with a tensor that never has a gradient), unclipped L2 wd
    0.01 at twice the lr.  The second group has no gradients at all in the
    fourth step, so its step count falls one behind the others'."""
    s = Setup(lr, sched, ema_decay)
    name = f"three_groups_vs_twin lr={lr:g}"
    for step in range(6):
        s.step_and_check(name, step, absent=(1,) if step == 3 else ())
    d = s.opt._dev["counters"].tolist()
    assert d[:3] == [6, 5, 6] and d[64] == 0
    assert [float(s.opt.state[ps[0]]["step"]) for ps in s.gp] == [6.0, 5.0, 6.0]
    assert not s.opt.state.get(s.gp[1][2])
    assert s.gp[0][2].data_ptr() % 16 == 4
    if ema_decay is not None:
        emas = s.opt.ema_parameters()
        flat = [p for ps in s.gp for p in ps]
        assert len(emas) == len(flat) and emas[5].data_ptr() == s.gp[1][2].data_ptr()
        trained = [p.detach().clone() for p in flat]
        versions = [p._version for p in flat]
        with s.opt.ema_weights():
            assert all(torch.equal(p.detach(), e) for p, e in zip(flat, emas))
            assert all(p._version > v for p, v in zip(flat, versions))
        assert all(torch.equal(bits(p), bits(t)) for p, t in zip(flat, trained))
    else:
        # state_dict interchange with torch.optim.AdamW
        ref = torch.optim.AdamW([{"params": [torch.nn.Parameter(p.detach().clone()) for p in ps]} for ps in s.gp],
                                lr=lr)
        ref.load_state_dict(s.opt.state_dict())


def test_only_ema_misaligned():
    """p, g and the moments 16-byte aligned, ema a view 4 bytes off: the
    element pass takes its scalar path beside sumsq's vector path; the
    sentinels around the EMA view stay."""
    from mtts.optim import FusedClipAdamW
    n = CHUNK + 5
    gen = torch.Generator().manual_seed(0)
    init = torch.randn(n, generator=gen)
    groups = [dict(init=[init], lr=1e-2, wd=0.01, decoupled=True, clip=True)]
    p = torch.nn.Parameter(init.to(DEV))
    opt = FusedClipAdamW([p], lr=1e-2, betas=BETAS, eps=EPS, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9)
    twin = GroupTwin(groups, BETAS, EPS, 1.0, CONSTANT, 0.9)
    ebuf = torch.full((n + 10,), 12345.0, device=DEV)
    e = ebuf[1:1 + n]
    e.copy_(p.detach())
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p),
                    "ema": e}
    for step in range(2):
        g = torch.randn(n, generator=gen) * (3.0 if step else 0.01)
        p.grad = g.to(DEV)
        assert p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0 and e.data_ptr() % 16 == 4
        before, e_before = p.detach().clone(), e.clone()
        opt.step()
        ref_before, ref_e_before, total = twin.step([[g]])
        close(opt.last_grad_norm, total, rtol=1e-5, name="norm")
        record_adamw("only_ema_misaligned",
                     update=update_close(before, p, ref_before[0][0], twin.values()[0][0], name="p"),
                     ema=update_close(e_before, e, ref_e_before[0][0], twin.ema[0][0], name="ema"))
        assert float(ebuf[0]) == 12345.0 and bool((ebuf[1 + n:] == 12345.0).all())
    assert opt.state[p]["ema"].data_ptr() == ebuf.data_ptr() + 4


# ----------------------------------------------------------- bit-equality anchor
ANCHOR_SHAPES = [(CHUNK + 1,), (7,), (33, 5), (2 * CHUNK,), (1,)]


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("max_norm", [1.0, None])
def test_bit_identical_to_fused_clip_adam(max_norm, wd):
    """One group, constant schedule, decoupled=False, no EMA, no skip: the new
    entry computes what mtts_clip_adam computes, bit for bit, over four steps
    (aligned tensors and one offset view)."""
    from mtts.optim import FusedClipAdam, FusedClipAdamW
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(*s, generator=gen) for s in ANCHOR_SHAPES]

    def params():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        v = offset_view(VIEW_N)
        v.copy_(init[0][:VIEW_N])
        return ps + [torch.nn.Parameter(v)]

    a, b = params(), params()
    oa = FusedClipAdam(a, lr=1e-4, betas=BETAS, eps=EPS, weight_decay=wd, max_grad_norm=max_norm)
    ob = FusedClipAdamW(b, lr=1e-4, betas=BETAS, eps=EPS, weight_decay=wd, decoupled=False, max_grad_norm=max_norm)
    ga, gb = offset_view(VIEW_N), offset_view(VIEW_N)
    for step in range(4):
        grads = [torch.randn(p.shape, generator=gen) * (3.0 if step % 2 else 0.01) for p in a]
        for ps, gv in ((a, ga), (b, gb)):
            for p, g in zip(ps[:-1], grads):
                p.grad = g.to(DEV)
            gv.copy_(grads[-1])
            ps[-1].grad = gv
        oa.step()
        ob.step()
        if max_norm is not None:
            assert torch.equal(bits(oa.last_grad_norm), bits(ob.last_grad_norm))
        for i, (p, q) in enumerate(zip(a, b)):
            for what, x, y in (("p", p, q), ("exp_avg", oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]),
                               ("exp_avg_sq", oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])):
                assert torch.equal(bits(x), bits(y)), f"step {step} tensor {i} {what}"
    assert int(ob._dev["counters"][0]) == 4


def test_train_step_one_optimizer_bit_identical():
    """TrainStep(one_optimizer=True) against the default two FusedClipAdam on
    the gradients of the same backward (test_gpu_c5's small models), two steps:
    every parameter and moment bit-identical, and the clipped norm too, which
    needs the decoder's tensors first and in the same chunk order."""
    import copy
    import train_harness as th
    from test_gpu_c5 import SMALL
    torch.manual_seed(0)
    models = th.build_models(DEV, **SMALL)
    models_b = th.C5Models(*(copy.deepcopy(m) for m in models))
    sa, sb = th.TrainStep(models), th.TrainStep(models_b, one_optimizer=True)
    assert len(sb.opt.param_groups) == 2 and [g["clip"] for g in sb.opt.param_groups] == [True, False]
    for k in range(2):
        batch = th.synthetic_batch(2, DEV, T_text=12, T_codec=24, T_ref=16, d_style=SMALL["d_style"], seed=2 + k)
        total = sa.losses(batch)[0]
        sa.backward(total)
        for p, q in zip(sa.params, sb.params):
            q.grad = None if p.grad is None else p.grad.clone()
        assert any(p.grad is None for p in sa.params) and any(p.grad is not None for p in sa.params)
        sa.optimizer_step()
        sb.optimizer_step()
        assert torch.equal(bits(sa.opt_dec.last_grad_norm), bits(sb.opt.last_grad_norm))
        for i, (p, q) in enumerate(zip(sa.params, sb.params)):
            assert torch.equal(bits(p), bits(q)), f"step {k} parameter {i}"
            if p.grad is not None:
                oa = sa.opt_dec if p in sa.opt_dec.state else sa.opt_rest
                for key in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(bits(oa.state[p][key]), bits(sb.opt.state[q][key])), f"step {k} {key} {i}"
    assert sb.opt._dev["counters"][:2].tolist() == [2, 2]


# -------------------------------------------------------------- skip_nonfinite
@pytest.mark.parametrize("where", [(0, 1), (2, 0)], ids=["clipped", "unclipped"])
def test_skip_nonfinite(where):
    """An inf in a clipped (unclipped) gradient at the third step: nothing
    changes but `skipped_steps`, and the step after it equals a twin that never
    saw the bad one."""
    s = Setup(1e-2, COSINE, 0.9, skip_nonfinite=True)
    name = "skip_nonfinite"
    for step in range(2):
        s.step_and_check(name, step)
    bad = s.draw(2)
    bad[where[0]][where[1]].view(-1)[3] = float("inf")
    s.set_grads(bad)
    state = lambda: [bits(t) for ps in s.gp for p in ps for t in
                     ([p] + [s.opt.state[p][k] for k in ("exp_avg", "exp_avg_sq", "ema") if s.opt.state.get(p)])]
    snap = state()
    s.opt.step()
    assert all(torch.equal(a, b) for a, b in zip(state(), snap))
    d = s.opt._dev["counters"].tolist()
    assert d[:3] == [2, 2, 2] and int(s.opt.skipped_steps) == 1
    assert float(s.opt.state[s.gp[0][0]]["step"]) == 3.0       # the host ran ahead ...
    sd = s.opt.state_dict()                                     # ... until state_dict() / sync_steps()
    assert float(s.opt.state[s.gp[0][0]]["step"]) == 2.0 and float(sd["state"][0]["step"]) == 2.0
    for step in range(2, 4):
        s.step_and_check(name, step)
    assert s.opt._dev["counters"].tolist()[:3] == [4, 4, 4] and int(s.opt.skipped_steps) == 1


def test_non_finite_without_the_flag_as_fused_clip_adam():
    """skip_nonfinite off: a NaN gradient element gives a NaN norm and a NaN
    coefficient, and every parameter of the clipped groups turns NaN, as
    FusedClipAdam's do; the unclipped group (coef = 1) stays finite."""
    s = Setup(1e-2)
    s.step_and_check("non_finite_flag_off", 0)
    bad = s.draw(1)
    bad[0][1][70] = float("nan")
    s.set_grads(bad)
    s.opt.step()
    assert torch.isnan(s.opt.last_grad_norm)
    for gi in (0, 1):
        for p, g in zip(s.gp[gi], bad[gi]):
            assert g is None or torch.isnan(p).all()
    assert torch.isfinite(s.gp[2][0]).all()
    assert s.opt._dev["counters"].tolist()[:3] == [2, 2, 2] and int(s.opt.skipped_steps) == 0
