"""Per-request sampling in MambaTTSDecoder.generate (mtts/decode.py + the
per-row HIP sampler): per-row temperature / top-k / top-p / seed / length
cap and the repetition penalty, on the small decoder and conditioning of
tests/test_gpu_generate.py -- against the float64 reference sampler fed the
decode_step logits, for what must not recapture, for the scalar path left as
it was, and for the independence of a row from its neighbours."""
import numpy as np
import pytest
import torch

import sample_rows_ref as RR
from test_gpu_generate import B, DEV, V, _conds, _model

pytestmark = pytest.mark.gpu

MIXED = dict(temperature=[0.0, 0.8, 1.2], top_k=[0, 5, 0], top_p=[1.0, 0.9, 0.6], seed=[11, 12, 13])
PENALTY = [1.0, 1.3, 1.3]     # 1.3 already changes the penalised rows' tokens on this model (asserted below)
WINDOW = 8
N = 48


@pytest.mark.parametrize("mode,cd", [("graph", torch.bfloat16), ("eager", torch.bfloat16), ("graph", None)])
def test_mixed_rows_equal_reference_sampler_loop(mode, cd):
    m = _model(cd)                      # cd None: fp32, the generic step (no device position counter)
    m.decode_mode = mode
    text, z, mask = _conds()
    kw = dict(text_mask=mask, repetition_window=WINDOW, **MIXED)
    toks, lens = m.generate(text, z, N, repetition_penalty=PENALTY, **kw)
    assert toks.shape == (B, N) and toks.dtype == torch.int64 and lens.tolist() == [N] * B
    assert len(m._engine.gen_graphs) == (1 if mode == "graph" else 0)
    plain, _ = m.generate(text, z, N, repetition_penalty=1.0, **kw)
    assert torch.equal(plain[0], toks[0])                       # row 0: greedy, penalty 1.0 in both
    assert not torch.equal(plain[1], toks[1]) and not torch.equal(plain[2], toks[2])
    toks = toks.cpu().numpy()
    live = [True] * B
    with torch.no_grad():
        tok = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        states = [None] * 2
        for t in range(N):
            lg, states = m.decode_step(tok, text, z, states, t, text_mask=mask)
            _, acc = RR.sample_rows_ref(lg[:, 0].float().cpu().numpy(), draw=[t] * B, penalty=PENALTY, window=WINDOW,
                                        history=toks, col=t, **MIXED)
            for r in range(B):
                if not live[r]:
                    continue
                assert int(toks[r, t]) in acc[r], f"row {r} step {t}: {toks[r, t]} not in {sorted(acc[r])}"
                if len(acc[r]) > 1:
                    live[r] = False               # ambiguous: the two loops may part here
            tok = torch.from_numpy(toks[:, t:t + 1]).to(DEV)
    assert sum(live) >= B - 1, live


def test_new_per_row_values_do_not_capture_again():
    m = _model()
    text, z, mask = _conds()
    kw = dict(text_mask=mask, repetition_window=WINDOW)
    first, _ = m.generate(text, z, N, repetition_penalty=PENALTY, **kw, **MIXED)
    assert list(m._engine.gen_graphs) == [("rows", None, 0, WINDOW)]
    other, _ = m.generate(text, z, N, temperature=[0.9, 0.0, 0.7], top_k=[3, 0, 9], top_p=[0.8, 1.0, 1.0],
                          seed=torch.tensor([5, 6, 7]), repetition_penalty=[1.5, 1.0, 0.9], **kw)
    assert len(m._engine.gen_graphs) == 1 and not torch.equal(other, first)
    again, _ = m.generate(text, z, N, repetition_penalty=PENALTY, **kw, **MIXED)
    assert len(m._engine.gen_graphs) == 1 and torch.equal(again, first)
    # a scalar seed is row_seeds(seed, B); a scalar penalty alone selects the per-row path too
    from mtts import ops
    a, _ = m.generate(text, z, 12, temperature=0.9, seed=3, repetition_penalty=1.0, **kw)
    b, _ = m.generate(text, z, 12, temperature=0.9, seed=ops.row_seeds(3, B), repetition_penalty=1.0, **kw)
    assert torch.equal(a, b) and len(m._engine.gen_graphs) == 1


def test_scalar_path_untouched_by_a_rows_call():
    m = _model()
    text, z, mask = _conds()
    skw = dict(temperature=0.9, top_k=5, top_p=0.9, seed=77, text_mask=mask)
    before, _ = m.generate(text, z, N, **skw)
    assert list(m._engine.gen_graphs) == [(0.9, 5, 0.9, None, 0)]
    m.generate(text, z, N, text_mask=mask, repetition_penalty=PENALTY, repetition_window=WINDOW, **MIXED)
    assert set(m._engine.gen_graphs) == {(0.9, 5, 0.9, None, 0), ("rows", None, 0, WINDOW)}
    after, _ = m.generate(text, z, N, **skw)
    assert torch.equal(after, before) and len(m._engine.gen_graphs) == 2


def test_per_row_caps():
    m = _model()
    text, z, mask = _conds()
    pad = 2
    kw = dict(text_mask=mask, pad_id=pad, repetition_penalty=PENALTY, repetition_window=WINDOW, **MIXED)
    full, _ = m.generate(text, z, N, **kw)
    caps = [5, N, 17]
    toks, lens = m.generate(text, z, caps, **kw)
    assert lens.tolist() == caps and toks.shape == (B, N)
    for r, c in enumerate(caps):
        assert torch.equal(toks[r, :c], full[r, :c]), r
        assert bool((toks[r, c:] == pad).all()), r
    toks, lens = m.generate(text, z, torch.tensor([5, 9, 7]), check_every=2, **kw)
    assert lens.tolist() == [5, 9, 7] and toks.shape == (B, 9)
    for r, c in enumerate([5, 9, 7]):
        assert torch.equal(toks[r, :c], full[r, :c]) and bool((toks[r, c:] == pad).all()), r
    assert len(m._engine.gen_graphs) == 1


def test_rows_are_independent():
    m = _model()
    text, z, mask = _conds()
    kw = dict(text_mask=mask, top_k=MIXED["top_k"], top_p=MIXED["top_p"], repetition_penalty=PENALTY,
              repetition_window=WINDOW)
    a, _ = m.generate(text, z, N, temperature=[0.0, 0.8, 1.2], seed=[11, 12, 13], **kw)
    b, _ = m.generate(text, z, N, temperature=[0.0, 1.1, 1.2], seed=[11, 99, 13], **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


def test_with_ragged_prompt():
    m = _model()
    text, z, mask = _conds()
    prompt = torch.randint(0, V, (B, 7), generator=torch.Generator().manual_seed(3)).to(DEV)
    toks, lens = m.generate(text, z, [6, 4, 6], prompt_tokens=prompt, prompt_lengths=[3, 7, 5], text_mask=mask,
                            repetition_penalty=PENALTY, repetition_window=WINDOW, **MIXED)
    assert toks.shape == (B, 6) and lens.tolist() == [6, 4, 6]
    lg = m._engine.prefill_logits.float().cpu().numpy()
    # the window holds generated tokens only: the first draw sees no penalty, whatever the prompt
    _, acc = RR.sample_rows_ref(lg, draw=[0] * B, penalty=PENALTY, window=WINDOW, history=toks.cpu().numpy(), col=0,
                                **MIXED)
    assert all(int(toks[r, 0]) in acc[r] for r in range(B)), (toks[:, 0].tolist(), acc)


def test_errors_are_raised_up_front():
    m = _model()
    text, z, mask = _conds()
    for bad, name in ((dict(temperature=[1.0] * (B + 1)), "temperature"), (dict(top_k=[1] * (B + 1)), "top_k"),
                      (dict(seed=[1] * (B + 1)), "seed"), (dict(temperature=[1.0, -1.0, 1.0]), "temperature"),
                      (dict(top_p=[0.9, 0.0, 1.0]), "top_p"), (dict(repetition_penalty=0.0), "repetition_penalty"),
                      (dict(repetition_penalty=[1.0, 1.2, float("inf")]), "repetition_penalty"),
                      (dict(repetition_penalty=1.2, repetition_window=257), "repetition_window"),
                      (dict(top_k=[0, -1, 0]), "top_k"), (dict(top_k=[0.5, 1, 2]), "top_k")):
        with pytest.raises(ValueError, match=name):
            m.generate(text, z, 4, text_mask=mask, **bad)
    for caps in ([4, 0, 4], [4] * (B + 1)):
        with pytest.raises(ValueError, match="max_new_tokens"):
            m.generate(text, z, caps, text_mask=mask)
    assert m._engine is None or not m._engine.gen_graphs        # nothing was captured on the way to an error
    toks, lens = m.generate(text, z, [4, 2, 3], text_mask=mask, temperature=[0.0, 1.0, 1.0])
    assert toks.shape == (B, 4) and lens.tolist() == [4, 2, 3]
