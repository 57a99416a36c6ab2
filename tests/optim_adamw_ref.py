"""References for FusedClipAdamW (mtts/optim.py, csrc/optim.hip mtts_clip_adamw).

`GroupTwin` is the float64 twin: clip_grad_norm_ over the clipped groups only,
then torch.optim.AdamW (decoupled groups) or torch.optim.Adam (L2 groups), one
torch optimizer per group, each group's lr set to lr_g * f(t) from
`sched_factor` before every step; the EMA e += (1 - d_t)(p_new - e) in
float64.  t is one more than the most advanced group's step count, and a group
without gradients in a step does not advance (torch's own rule).

`Restated` is the kernel's arithmetic in float32 torch, with its device
counters, and the mutants the CPU tests must reject.

Both take the groups as a list of dicts {init: [tensors], lr, wd, decoupled,
clip} and per step a list (per group) of lists of gradients (None = no
gradient)."""
import math
import os

import torch

KINDS = ("constant", "cosine", "linear", "inverse_sqrt")


def sched_factor(kind, W, T, r, t):
    """f(t) at the 1-based step t, in Python floats (doubles)."""
    if t <= W:
        return t / W
    if kind == "constant":
        return 1.0
    if kind == "inverse_sqrt":
        return max(r, math.sqrt(max(W, 1) / t))
    x = min(1.0, (t - W) / (T - W))
    if kind == "cosine":
        return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * x))
    assert kind == "linear"
    return r + (1.0 - r) * (1.0 - x)


def ema_decay_at(decay, warmup, t):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


CONSTANT = ("constant", 0, 0, 0.0)


class GroupTwin:
    def __init__(self, groups, betas, eps, max_norm, sched=CONSTANT, ema_decay=None, ema_warmup=False):
        self.groups, self.max_norm, self.sched = groups, max_norm, sched
        self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
        self.params = [[torch.nn.Parameter(t.detach().cpu().double().clone()) for t in g["init"]] for g in groups]
        self.opts = [(torch.optim.AdamW if g["decoupled"] else torch.optim.Adam)(
            ps, lr=g["lr"], betas=betas, eps=eps, weight_decay=g["wd"]) for g, ps in zip(groups, self.params)]
        self.ema = [[p.detach().clone() for p in ps] for ps in self.params]
        self.gsteps = [0] * len(groups)
        self.lr = [g["lr"] for g in groups]          # lr_g * f(t) of the last step
        self.factor = None

    def step(self, grads):
        """Returns (parameters before, EMA before, norm over the clipped groups' gradients)."""
        before = [[p.detach().clone() for p in ps] for ps in self.params]
        ema_before = [[e.clone() for e in es] for es in self.ema]
        t = 1 + max(self.gsteps)
        self.factor = sched_factor(*self.sched, t)
        clipped = []
        for gi, (g, ps, gs) in enumerate(zip(self.groups, self.params, grads)):
            for p, gr in zip(ps, gs):
                p.grad = None if gr is None else gr.detach().cpu().double().clone()
                if gr is not None and g["clip"]:
                    clipped.append(p)
            self.lr[gi] = g["lr"] * self.factor
            self.opts[gi].param_groups[0]["lr"] = self.lr[gi]
            if any(gr is not None for gr in gs):
                self.gsteps[gi] += 1
        if self.max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(clipped, self.max_norm) if clipped else torch.zeros(())
        else:
            total = torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in clipped])) if clipped else torch.zeros(())
        for opt in self.opts:
            opt.step()
        if self.ema_decay is not None:
            d = ema_decay_at(self.ema_decay, self.ema_warmup, t)
            for ps, es, gs in zip(self.params, self.ema, grads):
                for p, e, gr in zip(ps, es, gs):
                    if gr is not None:
                        e.add_((1.0 - d) * (p.detach() - e))
        return before, ema_before, total

    def values(self):
        return [[p.detach() for p in ps] for ps in self.params]

    def moments(self, gi, i):
        st = self.opts[gi].state[self.params[gi][i]]
        return st["exp_avg"], st["exp_avg_sq"]


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


MUTANTS = ("l2_decay", "sched_off", "ema_old_p", "norm_all", "skip_advances")


class Restated:
    """mtts_clip_adamw in float32 torch: adamw_final_kernel's scalars (double,
    cast once) and adamw_elem.  The sums of g^2 are float32 (in torch's order,
    not the kernel's chunk order)."""

    def __init__(self, groups, betas, eps, max_norm, sched=CONSTANT, ema_decay=None, ema_warmup=False,
                 skip_nonfinite=False, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.groups, self.betas, self.eps, self.max_norm, self.sched = groups, betas, eps, max_norm, sched
        self.ema_decay, self.ema_warmup, self.skip_nonfinite, self.mutant = ema_decay, ema_warmup, skip_nonfinite, mutant
        self.ps = [[t.detach().float().clone() for t in g["init"]] for g in groups]
        self.ms = [[torch.zeros_like(t) for t in ps] for ps in self.ps]
        self.vs = [[torch.zeros_like(t) for t in ps] for ps in self.ps]
        self.es = [[t.clone() for t in ps] for ps in self.ps]
        self.gsteps = [0] * len(groups)
        self.skipped = 0
        self.lr = [None] * len(groups)
        self.norm = None

    def step(self, grads):
        m = self.mutant
        b1, b2, eps_f = f32(self.betas[0]), f32(self.betas[1]), f32(self.eps)
        s, rest = f32(0.0), f32(0.0)
        for g, gs in zip(self.groups, grads):
            for gr in gs:
                if gr is not None:
                    q = (gr.float() * gr.float()).sum()
                    if g["clip"] or m == "norm_all":
                        s = s + q
                    else:
                        rest = rest + q
        total = torch.sqrt(s)
        self.norm = total
        coef = f32(1.0)
        if self.max_norm is not None:
            coef = torch.clamp(f32(self.max_norm) / (total + f32(1e-6)), max=1.0)
        active = [any(gr is not None for gr in gs) for gs in grads]
        if self.skip_nonfinite and not torch.isfinite(s + rest):
            self.skipped += 1
            if m == "skip_advances":
                self.gsteps = [c + a for c, a in zip(self.gsteps, active)]
            return
        t = 1 + max(self.gsteps)
        f = sched_factor(*self.sched, t + 1 if m == "sched_off" else t)
        omd = f32(1.0 - ema_decay_at(self.ema_decay, self.ema_warmup, t)) if self.ema_decay is not None else None
        for gi, (g, gs) in enumerate(zip(self.groups, grads)):
            lr_t = f32(g["lr"]).item() * f
            self.lr[gi] = f32(lr_t)
            if not active[gi]:
                continue
            self.gsteps[gi] += 1
            tg = self.gsteps[gi]
            step_size = f32(lr_t / (1.0 - b1.item() ** tg))
            bc2_sqrt = f32(math.sqrt(1.0 - b2.item() ** tg))
            wd = f32(g["wd"])
            decoupled = g["decoupled"] and m != "l2_decay"
            decay = f32(1.0 - lr_t * wd.item())
            c = coef if g["clip"] else f32(1.0)
            for i, gr in enumerate(gs):
                if gr is None:
                    continue
                p, mo, v, e = self.ps[gi][i], self.ms[gi][i], self.vs[gi][i], self.es[gi][i]
                p_old = p.clone()
                if decoupled:
                    p.mul_(decay)
                x = gr.float() * c
                if not decoupled and g["wd"] != 0:
                    x = wd * p + x
                mo.copy_(b1 * mo + (1 - b1) * x)
                v.copy_(b2 * v + (1 - b2) * x * x)
                denom = torch.sqrt(v) / bc2_sqrt + eps_f
                p.sub_(step_size * (mo / denom))
                if omd is not None:
                    e.add_(omd * ((p_old if m == "ema_old_p" else p) - e))
                assert p.dtype == mo.dtype == v.dtype == e.dtype == x.dtype == torch.float32


# ------------------------------------------------------------- parity record
_ERRS = {}
QUANTITIES = ("update", "exp_avg", "exp_avg_sq", "norm", "last_lr", "ema")


def record_adamw(test, **errs):
    row = _ERRS.setdefault(test, {})
    for k, v in errs.items():
        assert k in QUANTITIES
        row[k] = max(row.get(k, 0.0), float(v))


def write_adamw_parity(path):
    """Append this process's rows to `path` (the header once)."""
    if not path or not _ERRS:
        return
    new = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, "a") as fh:
        if new:
            fh.write("# tests/test_gpu_optim_adamw.py, tests/test_gpu_optim_adamw_graph.py: max over a test's cases and\n"
                     "# steps, FusedClipAdamW on the GPU vs the float64 twin (tests/optim_adamw_ref.py GroupTwin).\n"
                     "# update, ema: max|d - d_ref| / max|d_ref| of the per-step delta, per tensor (bound 1e-2);\n"
                     "# exp_avg, exp_avg_sq, norm: max|err| / max|ref| (bound 1e-5); last_lr: relative (bound 1e-6)\n")
            fh.write(f"{'test':<44}" + "".join(f"{q:>12}" for q in QUANTITIES) + "\n")
        for test in sorted(_ERRS):
            row = _ERRS[test]
            fh.write(f"{test:<44}" + "".join(f"{row[q]:>12.3e}" if q in row else f"{'-':>12}" for q in QUANTITIES)
                     + "\n")
    _ERRS.clear()
