"""Ragged prompts in MambaTTSDecoder.generate (prompt_lengths) on the model of
tests/test_gpu_generate.py (d_model 64, 2 layers, 4 heads, d_ff 128, d_style
16, V 64, B 3, head weights x 8).  The reference for a row of length l is the
rectangular generate on prompt[:, :l]: the path that existed before per-row
lengths did."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, TT, V, TP = 3, 12, 64, 37
# The prompt seed of the greedy-continuation test: the first of 3, 4, 5, ...
# for which, with lengths [37, 2, 18], at least 2 of the 3 rows keep a
# reference top-2 logit gap above 1e-3 over all 16 steps.  It was determined
# on the rectangular code alone (the decode_step loop of
# test_prefill_greedy_continuation_fp32 per distinct length), before the
# ragged path was compared with anything.
GREEDY_SEED = 3
GREEDY_LENS = [37, 2, 18]


def _model(cd=torch.bfloat16, max_len=256):
    import mamba_decoder
    torch.manual_seed(0)
    m = mamba_decoder.MambaTTSDecoder(V, d_model=64, n_layers=2, n_heads=4, d_ff=128, d_style=16,
                                      max_len=max_len).to(DEV).eval()
    with torch.no_grad():
        m.head.weight.mul_(8.0)     # logits of order 1, so draws vary and greedy paths branch
    m.compute_dtype = cd
    return m


def _conds():
    g = torch.Generator().manual_seed(1)
    text = torch.randn(B, TT, 64, generator=g)
    z = torch.randn(B, 16, generator=g)
    mask = torch.ones(B, TT, dtype=torch.bool)
    mask[0, 9:] = False
    mask[2, 5:] = False
    return text.to(DEV), z.to(DEV), mask.to(DEV)


def _prompt(seed=3, tp=TP):
    return torch.randint(0, V, (B, tp), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _first_argmax(x):
    x = x.float()
    idx = torch.arange(x.shape[1], device=x.device).expand_as(x)
    return torch.where(x == x.max(1, keepdim=True).values, idx, x.shape[1]).min(1).values


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def _snapshot(m):
    eng = m._engine
    return [(a.clone(), b.clone()) for a, b in eng.states]


@functools.lru_cache(maxsize=None)
def _rect_reference(cd, length):
    """Today's rectangular generate(prompt[:, :length], 1 token): the prefill
    logits (for length 1: the first step's) and every layer's states after
    the prompt, computed once per (dtype, length) and shared."""
    m = _model(cd)
    text, z, mask = _conds()
    prompt = _prompt()[:, :length]
    if length > 1:
        m.generate(text, z, 1, prompt_tokens=prompt, temperature=0.0, text_mask=mask)
        return m._engine.prefill_logits.float().clone(), _snapshot(m)
    # one prompt token: nothing is prefilled; the states after the first step
    lg, states = m.decode_step(prompt, text, z, [None] * 2, 0, text_mask=mask)
    return lg[:, 0].float().clone(), [(a.clone(), b.clone()) for a, b in states]


@pytest.mark.parametrize("lens", [[37, 2, 18], [1, 37, 4]], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("cd,tol", [(None, 1e-3), (torch.bfloat16, 2e-2)], ids=["fp32", "bf16"])
def test_ragged_prefill_matches_rectangular_per_row(cd, tol, lens):
    m = _model(cd)
    text, z, mask = _conds()
    with torch.no_grad():
        m.generate(text, z, 1, prompt_tokens=_prompt(), prompt_lengths=lens, temperature=0.0, text_mask=mask)
        got_logits = m._engine.prefill_logits.float().clone()
        got_states = _snapshot(m)
        assert m._engine.pos32.tolist() == lens or m._engine.pos_buf.tolist() == lens   # len_b - 1, moved by the draw
        for b, n in enumerate(lens):
            ref_logits, ref_states = _rect_reference(cd, n)
            # (a one-token row: the rectangular run prefills nothing, so the ragged prefill, which
            # has consumed that token, is compared with the logits and states after the first step)
            e = _rel(got_logits[b], ref_logits[b])
            print(f"row {b} len {n}: prefill logits {e:.3e} of the scale")
            assert e <= tol, (b, n, e)
            for i, ((ca, sa), (cb, sb)) in enumerate(zip(got_states, ref_states)):
                ec, es = _rel(ca[b], cb[b]), _rel(sa[b], sb[b])
                print(f"row {b} len {n} layer {i}: conv state {ec:.3e}, ssm state {es:.3e} of the scale")
                assert ec <= tol and es <= tol, (b, n, i, ec, es)


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_padding_values_are_inert(mode):
    m = _model()
    m.decode_mode = mode
    text, z, mask = _conds()
    lens = [37, 2, 18]
    keep = torch.arange(TP, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None]
    base = _prompt()
    runs = []
    for fill in (torch.zeros_like(base), _prompt(seed=11), torch.full_like(base, -1)):
        p = torch.where(keep, base, fill)
        toks, n = m.generate(text, z, 12, prompt_tokens=p, prompt_lengths=lens, temperature=0.7, top_k=8, seed=5,
                             text_mask=mask)
        assert toks.shape == (B, 12) and n.tolist() == [12] * B
        runs.append(toks)
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    with pytest.raises(IndexError):     # ... but a bad id INSIDE a row's length still raises
        bad = base.clone()
        bad[1, 1] = V
        m.generate(text, z, 2, prompt_tokens=bad, prompt_lengths=lens, text_mask=mask)


def test_ragged_greedy_continuation_fp32():
    text, z, mask = _conds()
    prompt = _prompt(GREEDY_SEED)
    lens = GREEDY_LENS
    m = _model(None)
    toks, n = m.generate(text, z, 16, prompt_tokens=prompt, prompt_lengths=lens, temperature=0.0, text_mask=mask)
    assert toks.shape == (B, 16) and n.tolist() == [16] * B
    ok, refs = [True] * B, [None] * B
    ref_m = _model(None)
    for b, ln in enumerate(lens):
        # the rectangular run of this row's length, and its top-2 gaps from the decode_step loop
        refs[b], _ = ref_m.generate(text, z, 16, prompt_tokens=prompt[:, :ln], temperature=0.0, text_mask=mask)
        with torch.no_grad():
            states = [None] * 2
            for t in range(ln):
                lg, states = ref_m.decode_step(prompt[:, t:t + 1], text, z, states, t, text_mask=mask)
            for i in range(16):
                top2 = lg[b, 0].float().topk(2).values
                ok[b] = ok[b] and float(top2[0] - top2[1]) > 1e-3
                tok = _first_argmax(lg[:, 0])[:, None]
                lg, states = ref_m.decode_step(tok, text, z, states, ln + i, text_mask=mask)
    assert sum(ok) >= 2, ok
    for b in range(B):
        if ok[b]:
            assert torch.equal(toks[b], refs[b][b]), (b, toks[b].tolist(), refs[b][b].tolist())


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_equal_lengths_take_the_rectangular_path(mode):
    m = _model()
    m.decode_mode = mode
    text, z, mask = _conds()
    kw = dict(temperature=0.8, top_k=6, seed=9, text_mask=mask)
    for tp in (TP, 1):
        prompt = _prompt(tp=tp)
        plain, _ = m.generate(text, z, 10, prompt_tokens=prompt, **kw)
        same, _ = m.generate(text, z, 10, prompt_tokens=prompt, prompt_lengths=[tp] * B, **kw)
        assert torch.equal(plain, same)
    # lengths all equal but shorter than Tp: the rectangular run on the cut prompt
    prompt = _prompt()
    cut, _ = m.generate(text, z, 10, prompt_tokens=prompt[:, :20], **kw)
    same, _ = m.generate(text, z, 10, prompt_tokens=prompt, prompt_lengths=torch.full((B,), 20), **kw)
    assert torch.equal(cut, same)


def test_rectangular_and_ragged_replay_one_graph():
    m = _model()
    text, z, mask = _conds()
    kw = dict(temperature=0.8, top_k=6, text_mask=mask)
    prompt = _prompt()
    m.generate(text, z, 6, prompt_tokens=prompt, seed=1, **kw)
    eng = m._engine
    assert len(eng.gen_graphs) == 1
    (gr,) = eng.gen_graphs.values()
    rag, _ = m.generate(text, z, 6, prompt_tokens=prompt, prompt_lengths=[37, 2, 18], seed=1, **kw)
    assert m._engine is eng and len(eng.gen_graphs) == 1 and next(iter(eng.gen_graphs.values())) is gr
    # the replayed graph runs the ragged call as the eager engine does
    e = _model()
    e.decode_mode = "eager"
    rag_e, _ = e.generate(text, z, 6, prompt_tokens=prompt, prompt_lengths=[37, 2, 18], seed=1, **kw)
    assert torch.equal(rag, rag_e) and not e._engine.gen_graphs


def test_eos_on_a_ragged_prompt():
    m = _model()
    text, z, mask = _conds()
    prompt, lens = _prompt(), [37, 2, 18]
    free, _ = m.generate(text, z, 24, prompt_tokens=prompt, prompt_lengths=lens, temperature=0.0, text_mask=mask)
    free = free.tolist()
    # eos := the first token of row 1's greedy path that it had not emitted before (at column k >= 1), so
    # row 1 ends after k + 1 new tokens; row 0 is forced to end at its first; row 2 ends where its own
    # path first meets that token, if at all.  Until a row ends its path is the free one.
    k = next(i for i in range(1, 24) if free[1][i] not in free[1][:i])
    eos = free[1][k]
    pad = (eos + 1) % V
    bias = torch.zeros(B, V)
    bias[0] = float("-inf")
    bias[0, eos] = 0.0
    kw = dict(temperature=0.0, eos_id=eos, pad_id=pad, check_every=4, text_mask=mask)
    toks, n = m.generate(text, z, 24, prompt_tokens=prompt, prompt_lengths=lens, logit_bias=bias.to(DEV), **kw)
    want_n = [1, k + 1, free[2].index(eos) + 1 if eos in free[2] else 24]
    assert n.tolist() == want_n and len(set(want_n)) >= 2                # lengths count NEW tokens
    assert toks.shape == (B, max(want_n))
    for r, src in ((0, [eos]), (1, free[1]), (2, free[2])):
        row = src[:want_n[r]] + [pad] * (toks.shape[1] - want_n[r])      # the tail is pad_id
        assert toks[r].tolist() == row, r
    # rows that can never end keep the run going; ending rows are padded
    bias[:] = float("-inf")
    bias[:, eos] = 0.0
    bias[1, eos], bias[1, 7] = float("-inf"), 0.0
    t2, n2 = m.generate(text, z, 24, prompt_tokens=prompt, prompt_lengths=lens, logit_bias=bias.to(DEV), **kw)
    assert n2.tolist() == [1, 24, 1] and t2.shape == (B, 24)
    assert t2[1].tolist() == [7] * 24 and t2[2].tolist() == [eos] + [pad] * 23
    bias[1, eos], bias[1, 7] = 0.0, float("-inf")
    t3, n3 = m.generate(text, z, 24, prompt_tokens=prompt, prompt_lengths=lens, logit_bias=bias.to(DEV), **kw)
    assert n3.tolist() == [1, 1, 1] and t3.tolist() == [[eos]] * B       # trimmed where every row had finished


def test_ragged_errors():
    m = _model(max_len=64)
    text, z, mask = _conds()
    prompt = torch.zeros(B, 10, dtype=torch.long, device=DEV)
    for bad in ([0, 3, 10], [3, 11, 10], [3, 10], [[3, 3, 3]], torch.tensor([3.0, 4.0, 5.0])):
        with pytest.raises(ValueError):
            m.generate(text, z, 4, prompt_tokens=prompt, prompt_lengths=bad)
    with pytest.raises(ValueError):
        m.generate(text, z, 4, prompt_lengths=[1, 1, 1])           # lengths without a prompt
    with pytest.raises(IndexError):
        m.generate(text, z, 56, prompt_tokens=prompt, prompt_lengths=[10, 2, 5])   # 10 + 56 - 1 > 64
    toks, _ = m.generate(text, z, 55, prompt_tokens=prompt, prompt_lengths=[10, 2, 5], temperature=0.0)
    assert toks.shape == (B, 55)                                   # 10 + 55 - 1 == 64: the last position
    # the bound is the longest ROW, not the padded width
    toks, _ = m.generate(text, z, 58, prompt_tokens=prompt, prompt_lengths=[7, 2, 5], temperature=0.0)
    assert toks.shape == (B, 58)
    from mtts.mamba import Mamba
    mm = Mamba(64).to(DEV)
    with pytest.raises(RuntimeError):                              # seq_lens is inference only
        mm(torch.randn(B, 8, 64, device=DEV), seq_lens=[8, 2, 5])
    with torch.no_grad():
        out, (cs, ss) = mm(torch.randn(B, 8, 64, device=DEV), seq_lens=[8, 2, 5])
    assert out.shape == (B, 8, 64) and cs.shape == (B, 128, 4) and ss.shape == (B, 128, 16)


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("cd,tol", [(None, 1e-3), (torch.bfloat16, 2e-2)], ids=["fp32", "bf16"])
def test_decode_step_with_per_row_positions(cd, tol, mode):
    m = _model(cd)
    m.decode_mode = mode
    text, z, mask = _conds()
    seq = _prompt(seed=4, tp=4)
    with torch.no_grad():
        states = [None] * 2
        for t in range(3):
            _, states = m.decode_step(seq[:, t:t + 1], text, z, states, t, text_mask=mask)
        base = [(a.clone(), b.clone()) for a, b in states]
        fresh = lambda: [(a.clone(), b.clone()) for a, b in base]  # noqa: E731
        tok = seq[:, 3:4]
        # all-equal per-row positions: bitwise the int call
        lg_i, st_i = m.decode_step(tok, text, z, fresh(), 5, text_mask=mask)
        lg_i, st_i = lg_i.clone(), [(a.clone(), b.clone()) for a, b in st_i]
        lg_t, st_t = m.decode_step(tok, text, z, fresh(), torch.full((B,), 5, device=DEV), text_mask=mask)
        assert torch.equal(lg_t, lg_i)
        assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(st_t, st_i))
        # per-row positions against the int call at each row's position, from the same states
        pos = [5, 0, 3]
        lg_p, _ = m.decode_step(tok, text, z, fresh(), torch.tensor(pos), text_mask=mask)
        lg_p = lg_p.clone()
        for b, p in enumerate(pos):
            ref, _ = m.decode_step(tok, text, z, fresh(), p, text_mask=mask)
            e = _rel(lg_p[b, 0].float(), ref[b, 0].float())
            assert e <= tol, (b, p, e)
        assert not torch.equal(lg_p[1], lg_i[1])                   # the position does reach the logits
        with pytest.raises(IndexError):
            m.decode_step(tok, text, z, fresh(), torch.tensor([5, 256, 3]), text_mask=mask)
        with pytest.raises(IndexError):
            m.decode_step(tok, text, z, fresh(), torch.tensor([5, -1, 3]), text_mask=mask)
        with pytest.raises(ValueError):
            m.decode_step(tok, text, z, fresh(), torch.tensor([5, 3]), text_mask=mask)
