"""Cross-layer grouping of the deferred weight gradients (mtts/wgrad.py flush
policy, csrc/gemm.hip mtts_gemm_grouped_rounds) on test_gpu_wgrad.py's
d_model 256 decoder with 4 layers.

A layer of this model queues 9 jobs = 18 output tiles: 16 over K = B*T = 1024
tokens (16 K-tiles) and the 2 text-K/V tiles over K = 128 (2 K-tiles).  The
policy's group size (192 tiles, one C2 layer) is set to this model's 18 and
the CU count the policy sees to 16, so that rounds matter at this size as they
do at C2 on 256 CUs: one layer is a full round of long tiles with the short
ones on top (utilisation 260 / 288 = 0.90 < FILL), two layers are two rounds
(520 / 544 = 0.956): the policy flushes every two layers, 18 problems per
launch.  Same tile body and reduction order whatever the grouping: gradients
are bit-equal to per-layer flushing, and within 1e-4 of each tensor's scale
of the immediate path (split-K slabs: another summation order)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D, LAYERS, H, DFF, DS, T, TT, B = 256, 4, 4, 512, 16, 512, 64, 2
LAYER_TILES = 18


def _model(seed=0):
    import mamba_decoder
    torch.manual_seed(seed)
    m = mamba_decoder.MambaTTSDecoder(10, d_model=D, n_layers=LAYERS, n_heads=H, d_ff=DFF, d_style=DS,
                                      max_len=1024).cuda()
    m.compute_dtype = torch.bfloat16
    return m


def _batch(seed=7):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, 10, (B, T), generator=g).cuda()
    text = torch.randn(B, TT, D, generator=g).cuda()
    z = torch.randn(B, DS, generator=g).cuda()
    mask = torch.ones(B, TT, dtype=torch.bool).cuda()
    mask[0, 50:] = False
    return tok, text, z, mask


def _loss(m, tok, text, z, mask):
    from mtts.loss import cross_entropy
    logits = m(tok, text, z, text_mask=mask)
    return cross_entropy(logits.view(-1, 10), tok.view(-1), ignore_index=0)


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.fixture
def policy(monkeypatch):
    """The flush policy at this model's scale; records the launches' sizes."""
    from mtts import wgrad
    monkeypatch.setattr(wgrad, "MIN_GROUP_TILES", 0)
    monkeypatch.setattr(wgrad, "GROUP_TILES", LAYER_TILES)
    monkeypatch.setattr(wgrad, "_LAYER_TILES", LAYER_TILES)
    monkeypatch.setattr(wgrad, "cu_count", lambda dev: 16)
    launches = []
    real = wgrad._launch
    monkeypatch.setattr(wgrad, "_launch", lambda probs: launches.append(len(probs)) or real(probs))
    return launches


@pytest.fixture(scope="module")
def setup():
    """Model, batch and the immediate path's gradients (computed once)."""
    m = _model()
    batch = _batch()
    m.zero_grad(set_to_none=True)
    _loss(m, *batch).backward()
    return m, batch, _grads(m)


def _deferred_grads(m, batch):
    from mtts import wgrad
    m.zero_grad(set_to_none=True)
    with wgrad.deferred():
        _loss(m, *batch).backward()
    assert not wgrad._E.jobs and not wgrad._E.callback_queued
    return _grads(m)


def test_groups_fill_rounds_across_layers(setup, policy, monkeypatch):
    from mtts import wgrad
    m, batch, imm = setup
    monkeypatch.setattr(wgrad, "FILL_ROUNDS", False)
    per_layer = _deferred_grads(m, batch)
    assert policy == [9] * LAYERS, policy
    del policy[:]
    monkeypatch.setattr(wgrad, "FILL_ROUNDS", True)
    rounds = _deferred_grads(m, batch)
    assert len(policy) < LAYERS and policy == [18, 18], policy
    assert sum(policy) == 9 * LAYERS
    assert set(rounds) == set(per_layer) == set(imm)
    for n in rounds:
        assert torch.equal(rounds[n], per_layer[n]), n
        err = (rounds[n] - imm[n]).abs().max().item()
        scale = max(imm[n].abs().max().item(), 1e-6)
        assert err <= 1e-4 * scale, f"{n}: {err:.3e} > 1e-4 * {scale:.3e}"


def test_listener_keeps_per_layer_flushes(setup, policy):
    from mtts import wgrad
    m, batch, _ = setup
    seen = {}

    def fn(p):
        assert id(p) not in seen, "announced twice"
        seen[id(p)] = p.grad.detach().clone()
    wgrad.add_listener(fn)
    try:
        _deferred_grads(m, batch)
    finally:
        wgrad.remove_listener(fn)
    assert policy == [9] * LAYERS, policy                 # the per-layer flush points
    assert len(seen) == LAYERS * 8                         # the MHA in-projection weight once (two jobs)
    for p in m.parameters():
        if id(p) in seen:
            assert torch.equal(seen[id(p)], p.grad)


def test_graph_capture_replays_bit_equal(setup, policy):
    """A deferred backward (two 18-problem launches: the problem table travels
    in the kernel arguments) captured in a CUDA graph and replayed twice."""
    from mtts import wgrad
    m, batch, _ = setup
    eager = _deferred_grads(m, batch)
    n_eager = list(policy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _deferred_grads(m, batch)
    torch.cuda.current_stream().wait_stream(side)
    m.zero_grad(set_to_none=True)
    del policy[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with wgrad.deferred():
            _loss(m, *batch).backward()
    assert policy == n_eager == [18, 18]
    for _ in range(2):
        for p in m.parameters():
            if p.grad is not None:
                p.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = _grads(m)
        assert set(got) == set(eager)
        for n in got:
            assert torch.equal(got[n], eager[n]), n
    m.zero_grad(set_to_none=True)
