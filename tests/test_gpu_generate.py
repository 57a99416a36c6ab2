"""MambaTTSDecoder.generate (mtts/decode.py DecodeEngine.generate + the HIP
sampler) on the golden decoder's shape (d_model 64, 2 layers, 4 heads, d_ff
128, d_style 16), where the fused graph step applies: against the
decode_step loop it replaces, against the float64 reference sampler, and the
prompt prefill against decode_step on each prompt token in turn."""
import numpy as np
import pytest
import torch

import sample_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, TT, V = 3, 12, 64


def _model(cd=torch.bfloat16, max_len=256):
    import mamba_decoder
    torch.manual_seed(0)
    m = mamba_decoder.MambaTTSDecoder(V, d_model=64, n_layers=2, n_heads=4, d_ff=128, d_style=16,
                                      max_len=max_len).to(DEV).eval()
    with torch.no_grad():
        m.head.weight.mul_(8.0)     # logits of order 1, so draws vary and greedy paths branch
    m.compute_dtype = cd
    return m


def _conds(rows=slice(None)):
    g = torch.Generator().manual_seed(1)
    text = torch.randn(B, TT, 64, generator=g)
    z = torch.randn(B, 16, generator=g)
    mask = torch.ones(B, TT, dtype=torch.bool)
    mask[0, 9:] = False
    mask[2, 5:] = False
    return text[rows].to(DEV), z[rows].to(DEV), mask[rows].to(DEV)


def _first_argmax(x):
    """argmax with the lowest index on ties (torch.argmax where that is defined)."""
    x = x.float()
    idx = torch.arange(x.shape[1], device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, idx, x.shape[1]).min(1).values


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_greedy_equals_decode_step_argmax_loop(mode):
    m = _model()
    m.decode_mode = mode
    text, z, mask = _conds()
    toks, lens = m.generate(text, z, 48, temperature=0.0, text_mask=mask)
    assert toks.shape == (B, 48) and toks.dtype == torch.int64 and lens.tolist() == [48] * B
    if mode == "graph":
        assert m._engine is not None and len(m._engine.gen_graphs) == 1
        assert all(isinstance(g, torch.cuda.CUDAGraph) for g in m._engine.gen_graphs.values())
    else:
        assert not m._engine.gen_graphs
    with torch.no_grad():
        tok = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        states = [None] * 2
        for t in range(48):
            lg, states = m.decode_step(tok, text, z, states, t, text_mask=mask)
            tok = _first_argmax(lg[:, 0])[:, None]
            assert torch.equal(tok[:, 0], toks[:, t]), f"step {t}"
    assert len(torch.unique(toks)) > 3        # not a constant sequence
    # the same call again replays the cached graph and gives the same tokens
    again, _ = m.generate(text, z, 48, temperature=0.0, text_mask=mask)
    assert torch.equal(again, toks) and len(m._engine.gen_graphs) == (1 if mode == "graph" else 0)


def test_sampled_equals_reference_sampler_loop():
    m = _model()
    text, z, mask = _conds()
    kw = dict(temperature=0.9, top_k=5, top_p=0.9)
    toks, _ = m.generate(text, z, 48, text_mask=mask, seed=77, **kw)
    other, _ = m.generate(text, z, 48, text_mask=mask, seed=78, **kw)
    assert not torch.equal(other, toks) and len(m._engine.gen_graphs) == 1   # a new seed: no new capture
    toks = toks.cpu().numpy()
    live = [True] * B
    with torch.no_grad():
        tok = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        states = [None] * 2
        for t in range(48):
            lg, states = m.decode_step(tok, text, z, states, t, text_mask=mask)
            _, acc = SR.sample_ref(lg[:, 0].float().cpu().numpy(), seed=77, step=t, **kw)
            for r in range(B):
                if not live[r]:
                    continue
                assert int(toks[r, t]) in acc[r], f"row {r} step {t}: {toks[r, t]} not in {sorted(acc[r])}"
                if len(acc[r]) > 1:
                    live[r] = False               # ambiguous: the two loops may part here
            tok = torch.from_numpy(toks[:, t:t + 1]).to(DEV)
    assert sum(live) >= B - 1, live


def _prefill_vs_steps(cd, tol):
    m = _model(cd)
    text, z, mask = _conds()
    assert float(m.quant_embed.weight.detach().abs().max()) > 0     # untouched: prefill must not add it
    prompt = torch.randint(0, V, (B, 37), generator=torch.Generator().manual_seed(3)).to(DEV)
    m.generate(text, z, 1, prompt_tokens=prompt, temperature=0.0, text_mask=mask)
    eng = m._engine
    got_states = [(a.clone(), b.clone()) for a, b in eng.states]
    got_logits = eng.prefill_logits.float().clone()
    with torch.no_grad():
        states = [None] * 2
        for t in range(37):
            lg, states = m.decode_step(prompt[:, t:t + 1], text, z, states, t, text_mask=mask)
    e = _rel(got_logits, lg[:, 0].float())
    print(f"{cd}: prefill logits vs 37 decode_steps: {e:.3e} of the scale")
    assert e <= tol, e
    for i, ((ca, sa), (cb, sb)) in enumerate(zip(got_states, states)):
        ec, es = _rel(ca, cb), _rel(sa, sb)
        print(f"{cd}: layer {i} conv state {ec:.3e}, ssm state {es:.3e} of the scale")
        assert ec <= tol and es <= tol, (i, ec, es)


def test_prefill_states_and_logits_bf16():
    _prefill_vs_steps(torch.bfloat16, 2e-2)


def test_prefill_states_and_logits_fp32():
    _prefill_vs_steps(None, 1e-3)


def test_prefill_greedy_continuation_fp32():
    m = _model(None)
    text, z, mask = _conds()
    prompt = torch.randint(0, V, (B, 37), generator=torch.Generator().manual_seed(3)).to(DEV)
    toks, lens = m.generate(text, z, 16, prompt_tokens=prompt, temperature=0.0, text_mask=mask)
    assert toks.shape == (B, 16) and lens.tolist() == [16] * B
    ok = [True] * B
    with torch.no_grad():
        states = [None] * 2
        for t in range(37):
            lg, states = m.decode_step(prompt[:, t:t + 1], text, z, states, t, text_mask=mask)
        ref = []
        for i in range(16):
            top2 = lg[:, 0].float().topk(2, dim=1).values
            for r in range(B):
                ok[r] = ok[r] and float(top2[r, 0] - top2[r, 1]) > 1e-3
            tok = _first_argmax(lg[:, 0])[:, None]
            ref.append(tok)
            lg, states = m.decode_step(tok, text, z, states, 37 + i, text_mask=mask)
    ref = torch.cat(ref, 1)
    assert sum(ok) >= 2, ok
    for r in range(B):
        if ok[r]:
            assert torch.equal(toks[r], ref[r]), (r, toks[r].tolist(), ref[r].tolist())


def test_eos_padding_and_early_stop():
    m = _model()
    text, z, mask = _conds()
    eos, pad = 5, 2
    bias = torch.zeros(B, V)
    bias[:, eos] = float("-inf")
    bias[0] = float("-inf")
    bias[0, eos] = 0.0                                     # row 0 ends at its first step
    kw = dict(temperature=0.0, eos_id=eos, pad_id=pad, check_every=4)
    toks, lens = m.generate(text, z, 48, text_mask=mask, logit_bias=bias.to(DEV), **kw)
    assert toks.shape == (B, 48) and lens.tolist() == [1, 48, 48]
    assert toks[0].tolist() == [eos] + [pad] * 47
    # batch rows never mix: the other rows equal a run without row 0
    text2, z2, mask2 = _conds(slice(1, None))
    toks2, lens2 = m.generate(text2, z2, 48, text_mask=mask2, logit_bias=bias[1:].to(DEV), **kw)
    assert torch.equal(toks2, toks[1:]) and lens2.tolist() == [48, 48]
    # every row ends at once: the result is trimmed there, long before max_new_tokens
    bias[:] = float("-inf")
    bias[:, eos] = 0.0
    bias[1, eos], bias[1, 7] = float("-inf"), 0.0          # ... but row 1, which can only emit 7
    toks3, lens3 = m.generate(text, z, 200, text_mask=mask, logit_bias=bias.to(DEV), **kw)
    assert lens3.tolist() == [1, 200, 1] and toks3.shape == (B, 200)
    bias[1, eos], bias[1, 7] = 0.0, float("-inf")
    toks4, lens4 = m.generate(text, z, 200, text_mask=mask, logit_bias=bias.to(DEV), **kw)
    assert lens4.tolist() == [1, 1, 1] and toks4.tolist() == [[eos]] * B


def test_errors_are_raised_up_front():
    m = _model(max_len=64)
    text, z, mask = _conds()
    prompt = torch.zeros(B, 10, dtype=torch.long, device=DEV)
    with pytest.raises(IndexError):
        m.generate(text, z, 56, prompt_tokens=prompt)      # 10 + 56 - 1 > 64
    with pytest.raises(ValueError):
        m.generate(text, z, 4, pad_id=V)
    with pytest.raises(ValueError):
        m.generate(text, z, 4, eos_id=-1)
    with pytest.raises(ValueError):
        m.generate(text, z, 4, top_p=0.0)
    with pytest.raises(ValueError):
        m.generate(text, z, 4, temperature=-1.0)
    m.decode_mode = None
    with pytest.raises(RuntimeError):
        m.generate(text, z, 4)
    m.decode_mode = "graph"
    toks, _ = m.generate(text, z, 55, prompt_tokens=prompt, temperature=0.0)   # 10 + 55 - 1 == 64: the last position
    assert toks.shape == (B, 55)


def test_generate_does_not_disturb_decode_step():
    m, fresh = _model(), _model()
    text, z, mask = _conds()
    seq = torch.randint(0, V, (B, 6), generator=torch.Generator().manual_seed(4)).to(DEV)

    def run(model):
        out = []
        with torch.no_grad():
            states = [None] * 2
            for t in range(6):
                lg, states = model.decode_step(seq[:, t:t + 1], text, z, states, t, text_mask=mask)
                out.append(lg.clone())
        return torch.cat(out, 1)

    before = run(m)
    m.generate(text, z, 20, text_mask=mask, temperature=0.8, top_k=4, seed=5,
               prompt_tokens=seq[:, :3])
    after = run(m)
    assert torch.equal(after, before) and torch.equal(after, run(fresh))
