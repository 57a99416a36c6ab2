"""The fused clip + Adam step inside a replayed hipGraph (bench.py --graph:
forward, cross-entropy, deferred weight gradients and FusedClipAdam.step()
captured once and replayed), the only mode that relies on the device step
counter, the device-computed bias corrections and the captured descriptor
upload.

Every replay is compared with clip_grad_norm_ + torch.optim.Adam in float64
stepped with the same gradients: the update by test_optim_ref_cpu.update_close
(max|dp - dp_ref| <= 1e-2 * max|dp_ref| per tensor), the moments and the norm
at 1e-5.  The whole-step test also holds the replay's loss and gradients to
an eager twin model's on the same batch at 1e-3 (tests/test_gpu_c5.py's
tolerance; both run the same kernels, so this is a cap, not a measurement).
The host guards (no capture before an eager step, one capture per parameter
list, captured buffers owned by the optimizer) are checked with
torch.cuda.is_current_stream_capturing patched: no graph is replayed on
released memory.  Measured errors: profiles/optim_parity.txt."""
import copy
import gc
import weakref

import pytest
import torch

from test_gpu_ops import close, DEV
from test_gpu_optim import LR, check_after, draw, make, rand_grads
from test_optim_ref_cpu import record, ref_one_step, rel_err, update_close, write_parity

pytestmark = pytest.mark.gpu

SHAPES = [(65537,), (7,), (33, 5)]


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    write_parity()


def warm_up(fn, n=2):
    """n eager calls on a side stream, as torch's capture recipe asks and bench.py does."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(n):
            fn(k)
    torch.cuda.current_stream().wait_stream(side)


def dstep(opt):
    return int(opt.param_groups[0]["_dstep"].item())


def test_optimizer_only_graph():
    from mtts.optim import FusedClipAdam
    name = "optimizer_only_graph"
    gen, init, gp, opt, twin = make(SHAPES)
    for p in gp:
        p.grad = torch.zeros_like(p)          # static: refilled with copy_

    def one(run, tag):
        grads = draw(gen, SHAPES, tag, init)
        for p, g in zip(gp, grads):
            p.grad.copy_(g)
        before = [p.detach().clone() for p in gp]
        run()
        ref_before, total = twin.step(grads)
        check_after(name, opt, gp, before, twin, ref_before, total)

    warm_up(lambda k: one(opt.step, k))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for k in range(3):
        one(graph.replay, 2 + k)
    # the host's step count is the capture's until sync_steps() reads the device counter
    assert all(float(opt.state[p]["step"]) == 2.0 for p in gp)
    assert dstep(opt) == 5
    opt.sync_steps()
    assert all(float(opt.state[p]["step"]) == 5.0 for p in gp)
    # the checkpoint taken now continues in a fresh optimizer, and the captured one continues eagerly:
    # both take the twin's step 6
    gp2 = [torch.nn.Parameter(p.detach().clone()) for p in gp]
    opt2 = FusedClipAdam(gp2, lr=LR, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))     # as a checkpoint read back: its own tensors
    grads = rand_grads(gen, SHAPES, 5)
    for p, q, g in zip(gp, gp2, grads):
        p.grad.copy_(g)
        q.grad = g.to(DEV)
    before, before2 = [p.detach().clone() for p in gp], [p.detach().clone() for p in gp2]
    opt.step()
    opt2.step()
    ref_before, total = twin.step(grads)
    check_after(name, opt, gp, before, twin, ref_before, total)
    check_after(name, opt2, gp2, before2, twin, ref_before, total)
    assert dstep(opt) == 6 and dstep(opt2) == 6
    assert all(float(o.state[p]["step"]) == 6.0 for o, ps in ((opt, gp), (opt2, gp2)) for p in ps)


@pytest.mark.parametrize("cd", [torch.bfloat16, None], ids=["bf16", "fp32"])
def test_train_step_graph(cd):
    """bench.py train_bench's step() on the smoke-sized decoder: captured after
    two eager warm-ups, replayed three times on new tokens."""
    import mamba_decoder
    from mtts import wgrad
    from mtts.loss import cross_entropy
    from mtts.optim import FusedClipAdam
    name = f"train_step_graph {'bf16' if cd else 'fp32'}"
    vocab, B, T, Tt = 10, 2, 24, 12
    torch.manual_seed(0)

    def decoder():
        m = mamba_decoder.MambaTTSDecoder(vocab, d_model=64, n_layers=2, n_heads=4, d_ff=128, d_style=16,
                                          max_len=128).to(DEV)
        m.compute_dtype = cd
        return m

    model, twin = decoder(), decoder()
    params, tparams = list(model.parameters()), list(twin.parameters())
    opt = FusedClipAdam(params, lr=LR, max_grad_norm=1.0)
    gen = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, vocab, (B, T), generator=gen).to(DEV)      # static input
    text = torch.randn(B, Tt, 64, generator=gen).to(DEV)
    z = torch.randn(B, 16, generator=gen).to(DEV)
    mask = torch.ones(B, Tt, dtype=torch.bool, device=DEV)
    mask[:, 10:] = False

    def fwd_bwd(m, zero):
        logits = m(tokens, text, z, text_mask=mask)
        loss = cross_entropy(logits.view(-1, vocab), tokens.view(-1), ignore_index=0)
        zero()
        with wgrad.deferred():
            loss.backward()
        return loss

    def step():
        loss = fwd_bwd(model, lambda: opt.zero_grad(set_to_none=True))
        opt.step()
        return loss

    def new_tokens():
        tokens.copy_(torch.randint(0, vocab, (B, T), generator=gen))

    warm_up(lambda k: (new_tokens(), step()))
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    live = [i for i, p in enumerate(params) if p.grad is not None]
    assert live
    losses = []
    for k in range(3):
        new_tokens()
        with torch.no_grad():
            for q, p in zip(tparams, params):
                q.copy_(p)
        before = [params[i].detach().clone() for i in live]
        m0 = [opt.state[params[i]]["exp_avg"].clone() for i in live]
        v0 = [opt.state[params[i]]["exp_avg_sq"].clone() for i in live]
        ref_loss = fwd_bwd(twin, lambda: twin.zero_grad(set_to_none=True))
        graph.replay()
        close(static_loss, ref_loss.detach(), rtol=1e-3, name=f"{name} loss replay {k}")
        errs = {"graph_loss": rel_err(static_loss, ref_loss.detach()), "graph_grad": 0.0, "update": 0.0,
                "exp_avg": 0.0, "exp_avg_sq": 0.0}
        for i, (p, q) in enumerate(zip(params, tparams)):
            assert (p.grad is None) == (q.grad is None) == (i not in live)
            if p.grad is not None:
                close(p.grad, q.grad, rtol=1e-3, name=f"{name} grad{i} replay {k}")
                errs["graph_grad"] = max(errs["graph_grad"], rel_err(p.grad, q.grad))
        ref_p, ref_m, ref_v, total = ref_one_step(before, [params[i].grad for i in live], m0, v0, 2 + k, LR, 0.0, 1.0,
                                                  betas=(0.9, 0.999))
        close(opt.last_grad_norm, total, rtol=1e-5, name=f"{name} norm replay {k}")
        errs["norm"] = rel_err(opt.last_grad_norm, total)
        for j, i in enumerate(live):
            st = opt.state[params[i]]
            errs["update"] = max(errs["update"], update_close(before[j], params[i], before[j], ref_p[j],
                                                              name=f"{name} param{i} replay {k}"))
            close(st["exp_avg"], ref_m[j], rtol=1e-5, name=f"{name} m{i} replay {k}")
            close(st["exp_avg_sq"], ref_v[j], rtol=1e-5, name=f"{name} v{i} replay {k}")
            errs["exp_avg"] = max(errs["exp_avg"], rel_err(st["exp_avg"], ref_m[j]))
            errs["exp_avg_sq"] = max(errs["exp_avg_sq"], rel_err(st["exp_avg_sq"], ref_v[j]))
        record(name, **errs)
        losses.append(static_loss.detach().item())
    assert dstep(opt) == 5
    assert len(set(losses)) == 3, f"replays saw stale inputs: losses {losses}"


# ------------------------------------------------------------- host guards
def small():
    gen, init, gp, opt, twin = make([(7,), (33, 5)])
    for p in gp:
        p.grad = torch.randn_like(p)
    return gp, opt


def test_capture_before_an_eager_step_is_refused(monkeypatch):
    """Moments and the step counter created while capturing would be fill
    nodes of the graph: every replay would zero them.  step() refuses, before
    it allocates or launches anything."""
    gp, opt = small()
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="one eager step"):
            opt.step()
    assert torch.cuda.memory_allocated() == mem
    assert all(not opt.state[p] for p in gp) and "_dstep" not in opt.param_groups[0] and not opt._plans
    opt.step()                                 # the eager step it asks for
    assert all(float(opt.state[p]["step"]) == 1.0 for p in gp)


def test_capture_right_after_load_state_dict_is_refused(monkeypatch):
    """load_state_dict drops the device step counter (re-seeded by the next
    eager step): a capture straight after it would reset the count at every replay."""
    gp, opt = small()
    opt.step()
    opt.load_state_dict(opt.state_dict())
    assert "_dstep" not in opt.param_groups[0]
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="one eager step"):
            opt.step()
    assert "_dstep" not in opt.param_groups[0] and not opt._plans
    opt.step()
    assert dstep(opt) == 2


def test_second_capture_of_a_parameter_list_is_refused(monkeypatch):
    gp, opt = small()
    warm_up(lambda k: opt.step(), n=1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="one captured graph per parameter list"):
            opt.step()
    assert dstep(opt) == 1


def test_captured_buffers_live_as_long_as_the_optimizer(monkeypatch):
    """A replay uploads from the captured plan's pinned buffer and runs on its
    device buffers.  The plan cache (cleared beyond 8 plans, replaced by
    load_state_dict) must not be their only owner: they stay alive, by
    weakref, after both.  (No graph is replayed here.)"""
    gp, opt = small()
    opt.step()
    with monkeypatch.context() as mp:          # the capture branch of _plan, run eagerly
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        opt.step()
    (plan,) = opt._plans.values()
    assert plan.get("captured") is not None
    refs = {k: weakref.ref(plan[k]) for k in ("cap_host", "captured", "ws", "norm")}
    refs["dstep"] = weakref.ref(opt.param_groups[0]["_dstep"])
    ptrs = {k: r().data_ptr() for k, r in refs.items()}
    del plan
    sd = opt.state_dict()
    for _ in range(10):                        # new moment tensors: a new plan each step
        for p in gp:
            st = opt.state[p]
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        opt.step()
    assert len(opt._plans) < 10                # the cache was cleared on the way
    assert all(pl.get("captured") is None for pl in opt._plans.values())
    gc.collect()
    assert all(r() is not None for r in refs.values()), "released with the plan cache"
    opt.load_state_dict(sd)
    assert not opt._plans
    gc.collect()
    assert all(r() is not None and r().data_ptr() == ptrs[k] for k, r in refs.items()), "released by load_state_dict"
