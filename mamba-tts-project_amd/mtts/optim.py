"""Optimizer step of the training loop (reference train.py:232-235:
clip_grad_norm_(decoder.parameters(), 1.0); optim.step() with
torch.optim.Adam(lr)).

FusedClipAdam is torch.optim.Adam (same hyper-parameters, same state names
`step` / `exp_avg` / `exp_avg_sq`, so state_dicts interchange) whose step()
also applies clip_grad_norm_(params, max_grad_norm) -- in three HIP launches
for the whole parameter list (mtts_clip_adam: partial sums of g^2, the norm
and clip coefficient on device, then Adam on g * coef).  Gradients are left
unclipped; `last_grad_norm` holds the total norm (device scalar).  The step
count is kept on the device too, so a training step that ends in step()
can be captured in a hipGraph (bench.py --graph).  A capture needs one eager
step() before it (on the same parameters, and again after load_state_dict):
the moments, the device step counter and the descriptor plan are created
eagerly, never as nodes of the graph, where every replay would zero them
again; step() raises otherwise.  What a captured graph reads and writes at
every replay (descriptors, workspace, norm, step counter) lives as long as
the optimizer.  A non-finite gradient norm gives a NaN clip coefficient, as
clip_grad_norm_'s clamp does: every parameter of the group turns NaN.

FusedClipAdamW (mtts_clip_adamw, the same three launches) is the optimizer for
real runs: parameter groups with decoupled or L2 weight decay, the clip over
the groups marked for it, a learning-rate schedule evaluated on the device,
EMA weights and a guard against non-finite gradients.  FusedClipAdam stays
as it is; with one L2 group the two are bit-identical.

clip_into_optimizer is the torch-optimizer variant (norm by foreach, the
clip folded into a fused torch Adam via grad_scale).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import torch

from . import _lib as L


def dense(t: torch.Tensor) -> bool:
    """t covers its storage span without gaps or overlap (a permutation of a
    contiguous tensor)."""
    if t.is_contiguous():
        return True
    order = sorted(range(t.dim()), key=lambda d: -t.stride(d))
    return t.permute(order).is_contiguous()


def same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal shapes and strides (a size-1 dimension's stride does not matter)."""
    return a.shape == b.shape and all(n == 1 or sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()))


NEEDS_EAGER_STEP = ("FusedClipAdam: take one eager step() before capturing (after construction and after "
                    "load_state_dict): the moments, the device step counter and the descriptor plan must exist "
                    "before the capture, or every replay would reset them")


class FusedClipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        if max_grad_norm is not None and len(self.param_groups) > 1:
            raise ValueError("FusedClipAdam: clipping spans one parameter group")
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self._plans = {}
        # (plan, step counter) of every captured step: a replay uploads from the
        # plan's pinned buffer and runs on its device buffers, so neither the
        # plan cache's eviction nor load_state_dict may release them
        self._captured = []

    def _plan(self, ps, dev, dstep=None):
        """Device descriptor array of (p, g, exp_avg, exp_avg_sq).  Parameters
        and moments are fixed; gradients may move between steps (zero_grad
        set_to_none), so a changed list is re-uploaded from a pinned buffer
        with an asynchronous copy (no host stall)."""
        # the descriptors hold raw pointers of p AND of its moments: key on
        # both, so replaced state tensors (load_state_dict) get a new plan
        pkey = tuple((p.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr())
                     for p in ps)
        gkey = tuple(p.grad.data_ptr() for p in ps)
        plan = self._plans.get(pkey)
        lib = L.lib()
        if plan is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(NEEDS_EAGER_STEP)
            ts = (L.AdamTensor * len(ps))()
            c0 = 0
            for i, p in enumerate(ps):
                st = self.state[p]
                ts[i].p = p.data_ptr()
                ts[i].m, ts[i].v = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                ts[i].n, ts[i].chunk0 = p.numel(), c0
                c0 += lib.mtts_adam_chunks(p.numel())
            nbytes = len(bytes(ts))
            plan = {"ts": ts, "nch": c0, "gkey": None, "uploads": 0,
                    "host": torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                    "cap_host": torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                    "dev": torch.empty(nbytes, dtype=torch.uint8, device=dev),
                    "ws": torch.empty(lib.mtts_adam_workspace(c0), device=dev, dtype=torch.uint8),
                    "norm": torch.zeros(4, device=dev, dtype=torch.float32), "ev": torch.cuda.Event()}
            if len(self._plans) > 8:
                self._plans.clear()
            self._plans[pkey] = plan
        if torch.cuda.is_current_stream_capturing():
            # hipGraph capture: the gradients live in the graph's pool at fixed
            # addresses; the descriptors go into a pinned buffer reserved for
            # the capture (allocated before it; nothing rewrites it later), and
            # its upload is a captured copy
            if plan.get("captured") is not None:     # a tensor: its truth value would raise instead
                raise RuntimeError("FusedClipAdam: one captured graph per parameter list")
            ts = plan["ts"]
            for i, p in enumerate(ps):
                ts[i].g = p.grad.data_ptr()
            plan["cap_host"].numpy()[:] = memoryview(bytes(ts))
            dev_buf = torch.empty(plan["cap_host"].numel(), dtype=torch.uint8, device=dev)
            dev_buf.copy_(plan["cap_host"], non_blocking=True)
            plan["captured"] = dev_buf
            self._captured.append((plan, dstep))
            return dev_buf, plan["nch"], plan["ws"], plan["norm"]
        if plan["gkey"] != gkey:
            ts = plan["ts"]
            for i, p in enumerate(ps):
                ts[i].g = p.grad.data_ptr()
            plan["ev"].synchronize()          # the previous upload has left the pinned buffer
            plan["host"].numpy()[:] = memoryview(bytes(ts))
            plan["dev"].copy_(plan["host"], non_blocking=True)
            plan["ev"].record()
            plan["gkey"] = gkey
            plan["uploads"] += 1
        return plan["dev"], plan["nch"], plan["ws"], plan["norm"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                if p.dtype != torch.float32 or not p.is_cuda or p.grad.dtype != torch.float32:
                    raise TypeError("FusedClipAdam takes fp32 CUDA (HIP) parameters and gradients")
                # the kernel walks storage order: p, grad and moments need one
                # dense layout (contiguous, or e.g. a conv weight kept [O][K][C])
                if p.grad.is_sparse or not dense(p) or not same_layout(p.grad, p):
                    raise ValueError("FusedClipAdam needs dense parameters and gradients of the same strides")
                st = self.state[p]
                if capturing and (not st or group.get("_dstep") is None):
                    # created here they would be fills inside the graph: every
                    # replay would zero the moments / reset the step counter
                    raise RuntimeError(NEEDS_EAGER_STEP)
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            steps = {float(self.state[p]["step"]) for p in ps}
            if len(steps) != 1:
                raise ValueError("FusedClipAdam: parameters of a group must share the step count")
            # the step count lives on the device (the kernels derive the bias
            # corrections from it), so a captured hipGraph of the whole training
            # step replays correctly; state["step"] mirrors it on the host in
            # eager mode (sync_steps() after graph replays)
            dstep = group.get("_dstep")
            if dstep is None:
                dstep = torch.full((1,), int(steps.pop()), device=ps[0].device, dtype=torch.int32)
                group["_dstep"] = dstep
            if not capturing:
                for p in ps:
                    self.state[p]["step"] += 1
            raw, nch, ws, norm = self._plan(ps, ps[0].device, dstep)
            b1, b2 = group["betas"]
            mx = float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0
            L.call_raw("mtts_clip_adam", raw.data_ptr(), len(ps), nch, dstep.data_ptr(), float(group["lr"]), float(b1),
                       float(b2), float(group["eps"]), float(group["weight_decay"]), mx, ws.data_ptr(), norm.data_ptr())
            self.last_grad_norm = norm[0]
        return loss

    def sync_steps(self):
        """Copy the device step counters into state["step"] (after replays)."""
        for group in self.param_groups:
            dstep = group.get("_dstep")
            if dstep is None:
                continue
            n = float(dstep.item())
            for p in group["params"]:
                if p in self.state and self.state[p]:
                    self.state[p]["step"].fill_(n)

    def state_dict(self):
        sd = super().state_dict()
        for g in sd["param_groups"]:
            g.pop("_dstep", None)
        return sd

    def load_state_dict(self, state_dict):
        """torch.optim.Adam.load_state_dict, then drop every cached descriptor
        plan (they point at the replaced moment tensors) and the device step
        counters (re-seeded from the loaded state["step"] on the next step).
        A graph captured before the load still steps the replaced moments:
        take one eager step and capture again."""
        super().load_state_dict(state_dict)
        self._plans = {}
        for g in self.param_groups:
            g.pop("_dstep", None)
        for st in self.state.values():
            # torch's loader may move "step" to the parameter's device; keep it a host scalar as __init__ does
            if "step" in st and torch.is_tensor(st["step"]) and st["step"].device.type != "cpu":
                st["step"] = st["step"].detach().cpu()


@torch.no_grad()
def clip_into_optimizer(optimizer, params, max_norm: float, eps: float = 1e-6):
    """Return the total gradient norm; arm `optimizer` (fused Adam/AdamW) to
    apply clip_grad_norm_'s scaling in its next step()."""
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return torch.zeros(())
    norms = torch._foreach_norm(grads, 2.0)
    total = torch.linalg.vector_norm(torch.stack([n.float() for n in norms]), 2.0)
    coef = torch.clamp(max_norm / (total + eps), max=1.0)
    scale = getattr(optimizer, "grad_scale", None)
    if scale is None or scale.device != total.device:
        optimizer.grad_scale = torch.empty((), device=total.device, dtype=torch.float32)
    optimizer.grad_scale.copy_(1.0 / coef)
    return total


# ---------------------------------------------------------------- FusedClipAdamW
class LRSchedule:
    """Learning-rate factor f(t) at the 1-based step t (include/mtts.h): linear
    warm-up t / W over the first W = warmup_steps steps, then by `kind` with
    x = min(1, (t - W) / (T - W)), T = total_steps, r = min_ratio: "constant"
    1; "cosine" r + (1 - r)(1 + cos(pi x)) / 2; "linear" r + (1 - r)(1 - x);
    "inverse_sqrt" max(r, sqrt(max(W, 1) / t)).  The device evaluates it from
    its own step counter; factor() is the same formula on the host."""

    def __init__(self, kind="constant", warmup_steps=0, total_steps=0, min_ratio=0.0):
        if kind not in L.LR_KINDS:
            raise ValueError(f"LRSchedule: kind {kind!r} is none of {sorted(L.LR_KINDS)}")
        if int(warmup_steps) != warmup_steps or int(total_steps) != total_steps or warmup_steps < 0:
            raise ValueError("LRSchedule: warmup_steps and total_steps are non-negative integers")
        if kind in ("cosine", "linear") and total_steps <= warmup_steps:
            raise ValueError(f"LRSchedule: {kind} needs total_steps > warmup_steps")
        if not 0.0 <= min_ratio <= 1.0:
            raise ValueError("LRSchedule: min_ratio outside [0, 1]")
        self.kind, self.warmup_steps, self.total_steps = kind, int(warmup_steps), int(total_steps)
        self.min_ratio = float(min_ratio)

    def factor(self, t: int) -> float:
        W, T, r = self.warmup_steps, self.total_steps, self.min_ratio
        if t <= W:
            return t / W
        if self.kind == "constant":
            return 1.0
        if self.kind == "inverse_sqrt":
            return max(r, math.sqrt(max(W, 1) / t))
        x = min(1.0, (t - W) / (T - W))
        if self.kind == "cosine":
            return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * x))
        return r + (1.0 - r) * (1.0 - x)


ADAMW_NEEDS_EAGER_STEP = NEEDS_EAGER_STEP.replace("FusedClipAdam:", "FusedClipAdamW:").replace(
    "the descriptor plan", "the group table and the descriptor plan")


class FusedClipAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW / Adam over parameter groups, with clip_grad_norm_
    over the groups marked `clip`, a learning-rate schedule evaluated on the
    device, EMA weights and a guard against non-finite gradients, in the three
    launches of mtts_clip_adamw for the whole list.

    Per-group keys: `lr`, `weight_decay`, `decoupled` (True: AdamW's
    p *= 1 - lr_t * wd; False: Adam's L2 g += wd * p) and `clip` (its
    gradients enter the norm and are scaled by the clip coefficient; the
    others are left as they are).  `betas` and `eps` are the optimizer's.
    `last_grad_norm` is the norm over the clipped groups, whether or not
    max_grad_norm is set.  State names are step / exp_avg / exp_avg_sq, plus
    `ema` with ema_decay; without EMA a state_dict interchanges with
    torch.optim.AdamW / Adam.

    Each group counts its own steps on the device (a group without gradients
    in a step does not advance, as in torch); the schedule and the EMA warm-up
    take t = 1 + the largest of those counts.  The group table (lr,
    weight_decay, decoupled, clip) lives on the device too: an eager step()
    re-uploads it when the host groups changed, update_hyper() does so on
    request, and a captured graph reads it at every replay, so a host-side lr
    change takes effect without a new capture.

    skip_nonfinite: a step whose sum of g^2 over all gradients is not finite in
    fp32 (NaN, inf, or an overflow of the sum over finite gradients) changes
    nothing and counts in `skipped_steps`; the host's state["step"] then runs
    ahead until sync_steps() (state_dict() calls it).

    The capture rules are FusedClipAdam's: one eager step before a capture
    (after construction and after load_state_dict), one captured graph per
    parameter list, sync_steps() after replays."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True,
                 max_grad_norm=None, schedule=None, ema_decay=None, ema_warmup=False, skip_nonfinite=False):
        if schedule is None:
            schedule = LRSchedule()
        elif isinstance(schedule, dict):
            schedule = LRSchedule(**schedule)
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError("FusedClipAdamW: ema_decay outside [0, 1)")
        self._ready = False
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled, clip=True)
        super().__init__(params, defaults)
        self._check_groups()
        self._ready = True
        self.max_grad_norm = max_grad_norm
        self.schedule = schedule
        self.ema_decay, self.ema_warmup, self.skip_nonfinite = ema_decay, bool(ema_warmup), bool(skip_nonfinite)
        self.last_grad_norm = self.last_lr = self.last_lr_factor = self.skipped_steps = None
        self._plans = {}
        self._dev = None           # device-side state shared by the plans: group table, counters
        self._captured = []        # what a captured graph reads and writes at replay: never released

    def _check_groups(self):
        groups = self.param_groups
        if len(groups) > L.ADAMW_MAX_GROUPS:
            raise ValueError(f"FusedClipAdamW: {len(groups)} parameter groups, at most {L.ADAMW_MAX_GROUPS}")
        for g in groups:
            if tuple(g["betas"]) != tuple(groups[0]["betas"]) or g["eps"] != groups[0]["eps"]:
                raise ValueError("FusedClipAdamW: betas and eps are per optimizer, not per group")
            for p in g["params"]:
                if p.dtype != torch.float32:
                    raise ValueError("FusedClipAdamW takes fp32 parameters")
                if p.is_sparse or p.layout != torch.strided or not dense(p):
                    raise ValueError("FusedClipAdamW needs dense parameters")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if self._ready:
            self._check_groups()
            self._plans, self._dev = {}, None

    # ------------------------------------------------------------ device state
    def _group_key(self):
        return tuple((float(g["lr"]), float(g["weight_decay"]), bool(g["decoupled"]), bool(g["clip"]))
                     for g in self.param_groups)

    def _device_state(self, dev):
        """Group table and counters, created by the first eager step: steps
        [0, 64) per group, seeded from the host's state["step"], and the
        skipped-step count at [64]."""
        if self._dev is None:
            steps = [0] * (L.ADAMW_MAX_GROUPS + 1)
            for gi, group in enumerate(self.param_groups):
                seen = [float(self.state[p]["step"]) for p in group["params"] if self.state.get(p)]
                steps[gi] = int(max(seen)) if seen else 0
            nbytes = C.sizeof(L.AdamWGroup) * L.ADAMW_MAX_GROUPS
            self._dev = {"counters": torch.tensor(steps, dtype=torch.int32).to(dev), "key": None,
                         "table": torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                         "host": torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True), "ev": torch.cuda.Event()}
            self.skipped_steps = self._dev["counters"][L.ADAMW_MAX_GROUPS]
        return self._dev

    def update_hyper(self):
        """Upload lr / weight_decay / decoupled / clip of the host groups into
        the device table (asynchronous copy on the current stream, not inside
        a capture).  A captured graph reads the table at replay."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedClipAdamW: update_hyper() between replays, not inside a capture")
        d = self._dev
        if d is None:
            return                 # the first step uploads
        key = self._group_key()
        table = (L.AdamWGroup * L.ADAMW_MAX_GROUPS)()
        for gi, (lr, wd, dec, clip) in enumerate(key):
            table[gi].lr, table[gi].weight_decay, table[gi].decoupled, table[gi].clip = lr, wd, dec, clip
        d["ev"].synchronize()      # the previous upload has left the pinned buffer
        d["host"].numpy()[:] = memoryview(bytes(table))
        d["table"].copy_(d["host"], non_blocking=True)
        d["ev"].record()
        d["key"] = key

    def _plan(self, live, dev):
        """Descriptors of the live (group index, parameter) pairs, tensors of
        clipped groups first so that they own the chunks [0, clip_chunks); the
        order within each half is the groups' and the parameters' own."""
        order = ([(gi, p) for gi, p in live if self.param_groups[gi]["clip"]]
                 + [(gi, p) for gi, p in live if not self.param_groups[gi]["clip"]])
        ema = self.ema_decay is not None
        pkey = tuple((gi, p.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                      self.state[p]["ema"].data_ptr() if ema else 0) for gi, p in order)
        gkey = tuple(p.grad.data_ptr() for _, p in order)
        plan = self._plans.get(pkey)
        capturing = torch.cuda.is_current_stream_capturing()
        if plan is None:
            if capturing:
                raise RuntimeError(ADAMW_NEEDS_EAGER_STEP)
            lib = L.lib()
            ts = (L.AdamWTensor * len(order))()
            c0 = clip_chunks = 0
            active = 0
            for i, (gi, p) in enumerate(order):
                st = self.state[p]
                ts[i].p, ts[i].exp_avg, ts[i].exp_avg_sq = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                ts[i].ema = st["ema"].data_ptr() if ema else None
                ts[i].n, ts[i].chunk0, ts[i].group = p.numel(), c0, gi
                c0 += lib.mtts_adam_chunks(p.numel())
                if self.param_groups[gi]["clip"]:
                    clip_chunks = c0
                active |= 1 << gi
            nbytes = len(bytes(ts))
            plan = {"ts": ts, "ps": [p for _, p in order], "nch": c0, "clip_chunks": clip_chunks, "active": active,
                    "gkey": None, "uploads": 0,
                    "host": torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                    "cap_host": torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                    "dev": torch.empty(nbytes, dtype=torch.uint8, device=dev),
                    "ws": torch.empty(lib.mtts_adam_workspace(c0), device=dev, dtype=torch.uint8),
                    "out": torch.zeros(L.ADAMW_OUT_FLOATS, device=dev, dtype=torch.float32),
                    "ev": torch.cuda.Event()}
            if len(self._plans) > 8:
                self._plans.clear()
            self._plans[pkey] = plan
        ts = plan["ts"]
        if capturing:
            # as FusedClipAdam._plan: the capture gets a pinned buffer of its own and a captured upload
            if plan.get("captured") is not None:
                raise RuntimeError("FusedClipAdamW: one captured graph per parameter list")
            for i, p in enumerate(plan["ps"]):
                ts[i].g = p.grad.data_ptr()
            plan["cap_host"].numpy()[:] = memoryview(bytes(ts))
            dev_buf = torch.empty(plan["cap_host"].numel(), dtype=torch.uint8, device=dev)
            dev_buf.copy_(plan["cap_host"], non_blocking=True)
            plan["captured"] = dev_buf
            self._captured.append((plan, self._dev))
            return dev_buf, plan
        if plan["gkey"] != gkey:
            for i, p in enumerate(plan["ps"]):
                ts[i].g = p.grad.data_ptr()
            plan["ev"].synchronize()          # the previous upload has left the pinned buffer
            plan["host"].numpy()[:] = memoryview(bytes(ts))
            plan["dev"].copy_(plan["host"], non_blocking=True)
            plan["ev"].record()
            plan["gkey"] = gkey
            plan["uploads"] += 1
        return plan["dev"], plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = [(gi, p) for gi, group in enumerate(self.param_groups) for p in group["params"] if p.grad is not None]
        if not live:
            return loss
        capturing = torch.cuda.is_current_stream_capturing()
        dev = live[0][1].device
        for gi, p in live:
            if not p.is_cuda or p.device != dev or p.grad.dtype != torch.float32:
                raise TypeError("FusedClipAdamW takes CUDA (HIP) parameters of one device and fp32 gradients")
            if p.grad.is_sparse or not dense(p) or not same_layout(p.grad, p):
                raise ValueError("FusedClipAdamW needs dense parameters and gradients of the same strides")
            if capturing and (not self.state[p] or self._dev is None):
                raise RuntimeError(ADAMW_NEEDS_EAGER_STEP)
        for gi, p in live:
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self.ema_decay is not None and "ema" not in st:
                if capturing:
                    raise RuntimeError(ADAMW_NEEDS_EAGER_STEP)
                st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
        for gi in {gi for gi, _ in live}:
            if len({float(self.state[p]["step"]) for g, p in live if g == gi}) != 1:
                raise ValueError("FusedClipAdamW: parameters of a group must share the step count")
        d = self._device_state(dev)
        if not capturing:
            if d["key"] != self._group_key():
                self.update_hyper()
            for _, p in live:
                self.state[p]["step"] += 1
        raw, plan = self._plan(live, dev)
        b1, b2 = self.param_groups[0]["betas"]
        a = L.AdamWArgs()
        a.beta1, a.beta2, a.eps = float(b1), float(b2), float(self.param_groups[0]["eps"])
        a.max_norm = float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0
        a.ngroups, a.ema_warmup, a.skip_nonfinite = len(self.param_groups), self.ema_warmup, self.skip_nonfinite
        a.ema_decay = float(self.ema_decay) if self.ema_decay is not None else 0.0
        a.active_groups, a.total_chunks, a.clip_chunks = plan["active"], plan["nch"], plan["clip_chunks"]
        s = self.schedule
        a.schedule.kind, a.schedule.warmup_steps = L.LR_KINDS[s.kind], s.warmup_steps
        a.schedule.total_steps, a.schedule.min_ratio = s.total_steps, s.min_ratio
        counters, out = d["counters"], plan["out"]
        L.call_raw("mtts_clip_adamw", raw.data_ptr(), len(live), d["table"].data_ptr(), C.byref(a),
                   counters.data_ptr(), counters.data_ptr() + 4 * L.ADAMW_MAX_GROUPS, plan["ws"].data_ptr(),
                   out.data_ptr())
        self.last_grad_norm, self.last_lr_factor = out[0], out[2]
        self.last_lr = out[L.ADAMW_OUT_LR:L.ADAMW_OUT_LR + len(self.param_groups)]
        return loss

    def sync_steps(self):
        """Copy the device step counters into state["step"] (after replays, or
        after skipped steps)."""
        if self._dev is None:
            return
        counts = self._dev["counters"].tolist()
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if self.state.get(p):
                    self.state[p]["step"].fill_(float(counts[gi]))

    def state_dict(self):
        if self.skip_nonfinite:
            self.sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch's load_state_dict, then drop every cached descriptor plan and
        the device counters and table (re-seeded from the loaded state by the
        next eager step).  A graph captured before the load still steps the
        replaced moments: take one eager step and capture again."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for k in ("decoupled", "clip"):     # a torch.optim.AdamW / Adam state_dict has neither
                g.setdefault(k, self.defaults[k])
        self._check_groups()
        self._plans, self._dev = {}, None
        self.skipped_steps = None
        for st in self.state.values():
            if "step" in st and torch.is_tensor(st["step"]) and st["step"].device.type != "cpu":
                st["step"] = st["step"].detach().cpu()

    # --------------------------------------------------------------------- EMA
    def ema_parameters(self):
        """The EMA tensors, aligned with the parameters in group order.  A
        parameter that has not stepped yet is its own average."""
        if self.ema_decay is None:
            raise RuntimeError("FusedClipAdamW: constructed without ema_decay")
        return [self.state[p]["ema"] if "ema" in self.state.get(p, {}) else p.detach()
                for group in self.param_groups for p in group["params"]]

    @contextlib.contextmanager
    def ema_weights(self):
        """Within the block the parameters hold their EMA values; the trained
        values come back on exit.  Both ways by copy_, which bumps the tensor
        versions, so caches keyed on them (decode contexts) rebuild."""
        ps = [p for group in self.param_groups for p in group["params"]]
        emas = self.ema_parameters()
        with torch.no_grad():
            saved = [p.detach().clone(memory_format=torch.preserve_format) for p in ps]
            for p, e in zip(ps, emas):
                p.copy_(e)
        try:
            yield
        finally:
            with torch.no_grad():
                for p, s in zip(ps, saved):
                    p.copy_(s)
