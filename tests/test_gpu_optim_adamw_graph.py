"""FusedClipAdamW.step() inside a replayed hipGraph: the mode that relies on
the device step counters, the schedule evaluated on the device and the group
table read at replay.  Captured after two eager steps with a three-step
warm-up, so the five replays cross the warm-up boundary; every replay is held
to the float64 twin as in test_gpu_optim_adamw (update and EMA delta by
update_close, moments and norm 1e-5, last_lr 1e-6).  update_hyper() between
replays changes a group's lr without a new capture.  The capture guards are
checked with torch.cuda.is_current_stream_capturing patched, as in
test_gpu_optim_graph: no graph is replayed on released memory."""
import copy
import gc
import os
import weakref

import pytest
import torch

from optim_adamw_ref import write_adamw_parity
from test_gpu_ops import DEV
from test_gpu_optim_adamw import COSINE, NO_GRAD, Setup, bits
from test_gpu_optim_graph import warm_up

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    write_adamw_parity(os.environ.get("MTTS_OPTIM_ADAMW_PARITY"))


def make_static(s):
    """Gradient tensors that stay where they are: refilled with copy_."""
    s.set_grads([[None if (gi, i) == NO_GRAD else torch.zeros(t.shape) for i, t in enumerate(g["init"])]
                 for gi, g in enumerate(s.groups)])
    s.static = True


def test_graph_replays_cross_the_warmup():
    name = "graph_replays"
    s = Setup(1e-2, COSINE, 0.9)
    make_static(s)
    warm_up(lambda k: s.step_and_check(name, k))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.opt.step()
    for k in range(2, 5):                      # t = 3 (the warm-up's last), 4, 5
        s.step_and_check(name, k, run=graph.replay)
    # a host-side lr change reaches the captured graph through the device table
    s.opt.param_groups[2]["lr"] *= 0.5
    s.groups[2]["lr"] *= 0.5                   # the twin's groups
    s.opt.update_hyper()
    for k in range(5, 7):
        s.step_and_check(name, k, run=graph.replay)
    assert abs(float(s.opt.last_lr[2]) / float(s.opt.last_lr[0]) - 1.0) < 1e-6      # 2 * 0.5
    # the host's step count is the capture's until sync_steps() reads the device counters
    flat = [p for ps in s.gp for p in ps if s.opt.state.get(p)]
    assert all(float(s.opt.state[p]["step"]) == 2.0 for p in flat)
    assert s.opt._dev["counters"].tolist()[:3] == [7, 7, 7]
    s.opt.sync_steps()
    assert all(float(s.opt.state[p]["step"]) == 7.0 for p in flat)
    # a checkpoint with EMA continues in a fresh optimizer: its eighth step equals the captured optimizer's eager
    # eighth step bit for bit, and that one is held to the twin
    sd = copy.deepcopy(s.opt.state_dict())
    s2 = Setup(1e-2, COSINE, 0.9)
    with torch.no_grad():
        for ps, qs in zip(s.gp, s2.gp):
            for p, q in zip(ps, qs):
                q.copy_(p)
    s2.opt.load_state_dict(sd)
    assert s2.opt.param_groups[2]["lr"] == s.opt.param_groups[2]["lr"] and s2.opt._dev is None
    grads = s.draw(7)
    s.set_grads(grads)
    s2.set_grads(grads)
    before, ema_before = s.snapshot()
    s.opt.step()
    s2.opt.step()
    s.check(name, grads, before, ema_before)
    for ps, qs in zip(s.gp, s2.gp):
        for p, q in zip(ps, qs):
            assert torch.equal(bits(p), bits(q))
            for key in ("exp_avg", "exp_avg_sq", "ema"):
                if s.opt.state.get(p):
                    assert torch.equal(bits(s.opt.state[p][key]), bits(s2.opt.state[q][key])), key
    assert s.opt._dev["counters"].tolist()[:3] == s2.opt._dev["counters"].tolist()[:3] == [8, 8, 8]


# ------------------------------------------------------------- host guards
def small(**kw):
    from mtts.optim import FusedClipAdamW
    gp = [torch.nn.Parameter(torch.randn(7, device=DEV)), torch.nn.Parameter(torch.randn(33, 5, device=DEV))]
    for p in gp:
        p.grad = torch.randn_like(p)
    return gp, FusedClipAdamW([{"params": gp[:1]}, {"params": gp[1:], "clip": False}], lr=1e-3, max_grad_norm=1.0, **kw)


def test_capture_before_an_eager_step_is_refused(monkeypatch):
    gp, opt = small(ema_decay=0.9)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="one eager step"):
            opt.step()
    assert torch.cuda.memory_allocated() == mem
    assert all(not opt.state[p] for p in gp) and opt._dev is None and not opt._plans
    opt.step()
    assert all(float(opt.state[p]["step"]) == 1.0 for p in gp)


def test_capture_right_after_load_state_dict_is_refused(monkeypatch):
    gp, opt = small()
    opt.step()
    opt.load_state_dict(opt.state_dict())
    assert opt._dev is None and not opt._plans
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="one eager step"):
            opt.step()
    assert opt._dev is None and not opt._plans
    opt.step()
    assert opt._dev["counters"].tolist()[:2] == [2, 2]


def test_second_capture_and_update_hyper_in_a_capture_are_refused(monkeypatch):
    gp, opt = small()
    warm_up(lambda k: opt.step(), n=1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="one captured graph per parameter list"):
            opt.step()
        with pytest.raises(RuntimeError, match="not inside a capture"):
            opt.update_hyper()
    assert opt._dev["counters"].tolist()[:2] == [1, 1]


def test_captured_buffers_live_as_long_as_the_optimizer(monkeypatch):
    """What a replay reads and writes (pinned descriptors, device descriptors,
    workspace, scalars, group table, counters) outlives the plan cache's
    eviction and load_state_dict.  (No graph is replayed here.)"""
    gp, opt = small()
    opt.step()
    with monkeypatch.context() as mp:          # the capture branch of _plan, run eagerly
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        opt.step()
    (plan,) = opt._plans.values()
    assert plan.get("captured") is not None
    refs = {k: weakref.ref(plan[k]) for k in ("cap_host", "captured", "ws", "out")}
    refs.update({k: weakref.ref(opt._dev[k]) for k in ("counters", "table")})
    ptrs = {k: r().data_ptr() for k, r in refs.items()}
    del plan
    sd = opt.state_dict()
    for _ in range(10):                        # new moment tensors: a new plan each step
        for p in gp:
            st = opt.state[p]
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        opt.step()
    assert len(opt._plans) < 10
    assert all(pl.get("captured") is None for pl in opt._plans.values())
    gc.collect()
    assert all(r() is not None for r in refs.values()), "released with the plan cache"
    opt.load_state_dict(sd)
    assert not opt._plans and opt._dev is None
    gc.collect()
    assert all(r() is not None and r().data_ptr() == ptrs[k] for k, r in refs.items()), "released by load_state_dict"
