"""Decode over a key side past the single-pass range (mtts/decode.py
OPTIONS["split_keys"], mtts_attention_decode_split): the packed step stays on,
the step equals the generic module path, a session request's tokens depend on
nothing but the request -- not its slot, its neighbours' key counts, what an
earlier request left in the slot's K / V rows, nor generate() versus session
-- and short conditioning runs exactly what it ran before.

The decoder is that of test_gpu_session.py's packed-step test (2 layers,
d_model 512, 8 heads: head dim 64, 256 keys per chunk) with max_keys =
2 * 256 + 8 = 520."""
import pytest
import torch

from test_gpu_generate import DEV, V
from test_gpu_generate_rows import WINDOW
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DM, DS, HEADS, SLOTS = 512, 16, 8, 20
CK = 256
KEYS = 2 * CK + 8
CAP = 20


def _decoder(cd):
    import mamba_decoder
    torch.manual_seed(0)
    m = mamba_decoder.MambaTTSDecoder(V, d_model=DM, n_layers=2, n_heads=HEADS, d_ff=512, d_style=DS,
                                      max_len=64).to(DEV).eval()
    m.compute_dtype = cd
    return m


@pytest.fixture(scope="module")
def model():
    from mtts.attn_kernels import decode_split_chunk
    assert decode_split_chunk(DM // HEADS) == CK
    return _decoder(torch.bfloat16)


def _req(keys, i, cap=CAP):
    """Request i over `keys` text keys: sampled, filtered, penalised (the controls of the session tests)."""
    g = torch.Generator().manual_seed(900 + 13 * i + keys)
    return dict(text_hidden=torch.randn(keys, DM, generator=g).to(DEV), z_style=torch.randn(DS, generator=g).to(DEV),
                max_new_tokens=cap, temperature=0.9, top_k=8, seed=40 + i, repetition_penalty=1.3)


def _solo(ses, slot, req):
    ses.admit(slot, **req)
    ses.run(req["max_new_tokens"])
    assert slot in ses.poll()
    return ses.take(slot)


def _generate_alone(m, req, keys=KEYS):
    S = req["text_hidden"].shape[0]
    text = torch.zeros(1, keys, DM, device=DEV)
    text[0, :S] = req["text_hidden"]
    mask = torch.zeros(1, keys, dtype=torch.bool, device=DEV)
    mask[0, :S] = True
    toks, lens = m.generate(text, req["z_style"][None], req["max_new_tokens"], text_mask=mask,
                            temperature=[req["temperature"]], top_k=[req["top_k"]], seed=[req["seed"]],
                            repetition_penalty=[req["repetition_penalty"]], repetition_window=WINDOW)
    assert lens.tolist() == [req["max_new_tokens"]]
    return toks[0]


def test_long_keys_keep_the_packed_step(model, monkeypatch):
    from mtts.decode import DecodeEngine
    assert DecodeEngine.OPTIONS["split_keys"] is True
    ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    assert ses.eng.ctx.fused and ses.eng.ctx.xpk and ses.cond.layers[0].khm is not None
    assert ses.eng.ctx.cond.kv_lens is ses.kv_lens and ses.kv_lens.dtype == torch.int32
    assert ses.kv_lens.tolist() == [1] * SLOTS              # an idle slot's only key is key 0
    assert not ses.eng.ctx.fuse_q
    monkeypatch.setitem(DecodeEngine.OPTIONS, "split_keys", False)
    old = model.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    assert old.eng.ctx.fused and not old.eng.ctx.xpk and old.cond.layers[0].khm is None


def _conds():
    g = torch.Generator(device=DEV).manual_seed(2)
    B = 3
    text = torch.randn(B, KEYS, DM, device=DEV, generator=g)
    z = torch.randn(B, DS, device=DEV, generator=g)
    mask = torch.ones(B, KEYS, dtype=torch.bool, device=DEV)
    mask[:, 100:131] = False                                # a hole: the padding of a reference prompt
    mask[1, 300:] = False                                   # ragged ends: 520, 300 and 257 keys
    mask[2, CK + 1:] = False
    tok = torch.randint(0, V, (B, 1), device=DEV, generator=g)
    return text, z, mask, tok


def _six_steps(m, mode, text, z, mask, tok):
    m.decode_mode = mode
    m.reset_decode_cache()
    states, seq = [None, None], []
    with torch.no_grad():
        for t in range(6):
            lg, states = m.decode_step(tok, text, z, states, t, text_mask=mask)
            seq.append(lg.float().clone())
    return torch.cat(seq, 1)


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_bf16_step_matches_the_module_path(model, mode):
    """Bound: 3e-2 of the logit scale, that of test_bf16_decode_engine_c4_shapes
    for the same comparison (bf16 roundings of the activations)."""
    text, z, mask, tok = _conds()
    try:
        got = _six_steps(model, mode, text, z, mask, tok)
        eng = model._engine
        assert eng.ctx.fused and eng.ctx.xpk and eng.ctx.cond.kv_lens.tolist() == [KEYS, 300, CK + 1]
        want = _six_steps(model, None, text, z, mask, tok)
    finally:
        model.decode_mode = "graph"
        model.reset_decode_cache()
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"bf16 engine ({mode}) vs module path at {KEYS} keys: {err:.3e} of the logit scale")
    close(got, want, rtol=3e-2, name=f"engine ({mode}) vs module path, {KEYS} keys")


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_fp32_step_matches_the_module_path(mode):
    """fp32: the generic step (_step) with the split kernel, at close()'s
    default bound, as test_decode_engine_matches_module_path's engine against
    its reference."""
    m = _decoder(None)
    text, z, mask, tok = _conds()
    got = _six_steps(m, mode, text, z, mask, tok)
    assert not m._engine.ctx.fused and m._engine.ctx.cond.kv_lens.tolist() == [KEYS, 300, CK + 1]
    want = _six_steps(m, None, text, z, mask, tok)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"fp32 engine ({mode}) vs module path at {KEYS} keys: {err:.3e} of the logit scale")
    close(got, want, name=f"fp32 engine ({mode}) vs module path, {KEYS} keys")


@pytest.mark.parametrize("keys", [5, CK, CK + 1, KEYS])
def test_a_request_of_any_key_count_runs_the_same_anywhere(model, keys):
    model.decode_mode = "graph"
    req = _req(keys, 0)
    others = [k for k in (5, CK, CK + 1, KEYS) if k != keys]
    ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    assert ses.eng.ctx.xpk
    want = _solo(ses, 1, req)                               # slot 1 of an otherwise idle session
    assert want.shape == (CAP,) and len(torch.unique(want)) > 3
    ses.admit(0, **_req(others[0], 1, cap=40))
    ses.admit(16, **_req(others[1], 2, cap=40))
    ses.admit(18, **_req(others[2], 3, cap=40))
    assert ses.kv_lens[[0, 16, 18]].tolist() == others
    ses.run(7)                                              # the neighbours are 7 tokens in
    assert torch.equal(_solo(ses, 17, req), want)           # the second half of the image, with neighbours
    longer = _solo(ses, 1, _req(KEYS, 4, cap=9))            # a longer request through slot 1 ...
    assert longer.shape == (9,) and ses.kv_lens[1].item() == 1
    assert torch.equal(_solo(ses, 1, req), want)            # ... and the slot right after it was taken
    assert ses.captures == 1
    assert torch.equal(_generate_alone(model, req), want)


def test_stale_keys_do_not_leak(model):
    model.decode_mode = "graph"
    ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    req = _req(5, 0)
    want = _solo(ses, 1, req)
    assert len(torch.unique(want)) > 3
    _solo(ses, 2, _req(KEYS, 4, cap=9))
    ses.admit(2, **req)
    assert ses.kv_lens[2].item() == 5
    for p in ses.cond.layers:                               # what the slot's rows hold past the request's keys
        p.k[2, 5:] = float("nan")
        p.v[2, 5:] = float("nan")
        p.khm[2, :, 5:] = float("nan")
        p.vhm[2, :, 5:] = float("nan")
    ses.run(CAP)
    assert 2 in ses.poll()
    assert torch.equal(ses.take(2), want)
    assert ses.captures == 1


def test_short_conditioning_is_untouched(model, monkeypatch):
    from mtts.decode import DecodeEngine
    model.decode_mode = "graph"
    req = _req(12, 0)
    runs = []
    for on in (True, False):
        monkeypatch.setitem(DecodeEngine.OPTIONS, "split_keys", on)
        ses = model.open_session(SLOTS, 16, repetition_window=WINDOW)
        assert ses.eng.ctx.xpk
        ses.admit(3, **req)
        ses.run(CAP)
        logits = ses.logits.clone()
        runs.append((ses.take(3), logits))
    assert len(torch.unique(runs[0][0])) > 3
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_routing_is_fixed_when_the_context_is_built(model, monkeypatch):
    """An engine that launches its step directly (no captured graph) keeps the
    routing its context was built with: the option switched afterwards changes
    neither the step in use nor a token."""
    from mtts.decode import DecodeEngine
    req = _req(CK + 1, 0)
    model.decode_mode = "eager"
    try:
        ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW)
        assert ses.captures == 0 and ses.eng.ctx.xpk and ses.cond.split is True
        want = _solo(ses, 1, req)
        monkeypatch.setitem(DecodeEngine.OPTIONS, "split_keys", False)
        assert torch.equal(_solo(ses, 1, req), want)        # still the packed step on the split kernel
        old = model.open_session(SLOTS, KEYS, repetition_window=WINDOW)
        assert not old.eng.ctx.xpk and old.cond.split is False
        monkeypatch.setitem(DecodeEngine.OPTIONS, "split_keys", True)
        assert _solo(old, 1, req).shape == (CAP,)           # still the parent's routing: no packed call is made
        assert old.cond.split_ws is None and ses.cond.split_ws is not None
    finally:
        model.decode_mode = "graph"
