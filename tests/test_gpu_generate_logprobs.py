"""Token log-probabilities through the engine: MambaTTSDecoder.generate(
return_logprobs=True), a decode session opened with logprobs=True and
generate_requests, on a small decoder (d_model 64, 2 layers, 4 heads, d_ff
128, d_style 16, max_len 256) with a vocabulary of 10 (the sampler's one-wave
form) and 300 (four waves), fp32 (the generic step) and bf16 (the fused step),
under a captured graph and launched directly.

generate(): the flag moves no token (on the fp32 step, where it also fixes
the row count of the BLAS projections, the logits of the two calls differ by
rounding and the tokens of these runs are still the same); columns at and past a row's length are
0.0; with a prompt, column 0 is the log-probability under the prefill logits;
graph and eager runs give the same bits; a repeat call captures nothing.
Session: after every run(1) the new column of every live slot is the reference
(tests/sample_logprob_ref.py) evaluated on session.logits of that step with
the controls, bias and history the test keeps itself, within lp_bound -- which
pins the column to the logits that produced the token; one request gives the
same bits in slot 1 of an idle session, in slot 17 beside live neighbours,
after another request left the slot, and in generate() at batch 1."""
import numpy as np
import pytest
import torch

import sample_logprob_ref as LP

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, TT, D, DS = 3, 12, 64, 16
KEYS, WINDOW, N = 16, 8, 24
LENS = (12, 9, 5)
MIXED = dict(temperature=[0.0, 0.8, 1.2], top_k=[0, 5, 0], top_p=[1.0, 0.9, 0.6], seed=[11, 12, 13])
PENALTY = [1.0, 1.3, 1.3]
SHAPES = [(10, None), (10, torch.bfloat16), (300, None), (300, torch.bfloat16)]
SHAPE_IDS = ["V10-fp32", "V10-bf16", "V300-fp32", "V300-bf16"]


def _model(V, cd, mode="graph"):
    import mamba_decoder
    torch.manual_seed(0)
    m = mamba_decoder.MambaTTSDecoder(V, d_model=D, n_layers=2, n_heads=4, d_ff=128, d_style=DS,
                                      max_len=256).to(DEV).eval()
    with torch.no_grad():
        m.head.weight.mul_(8.0)     # logits of order 1, so draws vary
    m.compute_dtype = cd
    m.decode_mode = mode
    return m


def _conds():
    g = torch.Generator().manual_seed(1)
    text = torch.randn(B, TT, D, generator=g)
    z = torch.randn(B, DS, generator=g)
    mask = torch.ones(B, TT, dtype=torch.bool)
    mask[0, 9:] = False
    mask[2, 5:] = False
    return text.to(DEV), z.to(DEV), mask.to(DEV)


def _bias(V, seed):
    """A request's logit bias: finite shifts and a forbidden fifth of the vocabulary."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(V, generator=g)
    b[torch.rand(V, generator=g) < 0.2] = float("-inf")
    b[seed % V] = 0.25
    return b.to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _valid(lp, lens):
    """(B, n) fp32: strictly negative, finite values inside a row's length, 0.0 at and past it."""
    assert lp.dtype == torch.float32
    inside = torch.arange(lp.shape[1], device=lp.device)[None, :] < lens[:, None]
    assert bool(torch.isfinite(lp).all()) and bool((lp[inside] < 0).all()) and bool((lp[~inside] == 0).all())


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("V,cd", SHAPES, ids=SHAPE_IDS)
def test_generate_returns_logprobs_and_moves_no_token(V, cd, mode):
    m = _model(V, cd, mode)
    text, z, mask = _conds()
    graphs = lambda: len(m._engine.gen_graphs)  # noqa: E731
    per_call = 1 if mode == "graph" else 0
    scalar = dict(text_mask=mask, temperature=0.9, top_k=5, top_p=0.95, seed=7)
    rows = dict(text_mask=mask, repetition_penalty=PENALTY, repetition_window=WINDOW, **MIXED)
    for kw in (scalar, rows):
        toks, lens = m.generate(text, z, N, **kw)
        assert m._engine.ctx.fused == (cd == torch.bfloat16)
        g0 = graphs()
        out = m.generate(text, z, N, return_logprobs=True, **kw)
        assert len(out) == 3 and graphs() == g0 + per_call                  # a graph of its own
        assert torch.equal(out[0], toks) and torch.equal(out[1], lens) and out[2].shape == (B, N)
        _valid(out[2], lens)
        again = m.generate(text, z, N, return_logprobs=True, **kw)
        assert graphs() == g0 + per_call                                    # replayed, not captured again
        assert torch.equal(again[0], toks) and torch.equal(_bits(again[2]), _bits(out[2]))
        assert len(torch.unique(out[2])) > N                                # values of their own per token
        # a token most rows emit as end of sequence: columns at and past a row's length hold 0.0
        eos = int(torch.mode(toks[:, 4:N - 4].flatten()).values)
        t2, l2 = m.generate(text, z, N, eos_id=eos, pad_id=1, **kw)
        o2 = m.generate(text, z, N, eos_id=eos, pad_id=1, return_logprobs=True, **kw)
        assert torch.equal(o2[0], t2) and torch.equal(o2[1], l2) and int(l2.min()) < N
        _valid(o2[2], l2)
        n = int(l2.min())
        assert torch.equal(_bits(o2[2][:, :n - 1]), _bits(out[2][:, :n - 1]))   # the same tokens from the same logits
    if mode == "graph":
        keys = set(m._engine.gen_graphs)
        assert {k for k in keys if k[-1] == "logprobs"} == {k + ("logprobs",) for k in keys if k[-1] != "logprobs"}
    # the flag off after it was on: the old return value
    assert len(m.generate(text, z, 4, **scalar)) == 2


@pytest.mark.parametrize("V,cd", SHAPES, ids=SHAPE_IDS)
def test_first_column_comes_from_the_prefill_logits(V, cd):
    m = _model(V, cd)
    text, z, mask = _conds()
    prompt = torch.randint(0, V, (B, 7), generator=torch.Generator().manual_seed(3)).to(DEV)
    bias = torch.stack([_bias(V, 20 + r) for r in range(B)])
    for kw in (dict(temperature=0.9, top_k=5, seed=7),
               dict(repetition_penalty=PENALTY, repetition_window=WINDOW, **MIXED)):
        toks, lens, lp = m.generate(text, z, 6, text_mask=mask, prompt_tokens=prompt, logit_bias=bias,
                                    return_logprobs=True, **kw)
        plain, _ = m.generate(text, z, 6, text_mask=mask, prompt_tokens=prompt, logit_bias=bias, **kw)
        assert torch.equal(plain, toks) and lp.shape == (B, 6)
        lg = m._engine.prefill_logits.float().cpu().numpy()                 # the draw count is 0: no penalty yet
        ref = LP.logprob_ref(lg, toks[:, 0].cpu().numpy(), bias=bias.cpu().numpy())
        for r in range(B):
            err = abs(float(lp[r, 0]) - ref[r])
            assert err <= LP.lp_bound(V, LP.threads_of(V), ref[r]), (r, float(lp[r, 0]), ref[r])
        _valid(lp, lens)


@pytest.mark.parametrize("V,cd", SHAPES, ids=SHAPE_IDS)
def test_graph_and_eager_give_the_same_bits(V, cd):
    text, z, mask = _conds()
    prompt = torch.randint(0, V, (B, 7), generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = (dict(temperature=0.9, top_k=5, seed=7),
             dict(repetition_penalty=PENALTY, repetition_window=WINDOW, **MIXED),
             dict(repetition_penalty=PENALTY, repetition_window=WINDOW, prompt_tokens=prompt, **MIXED))
    got = []
    for mode in ("graph", "eager"):
        m = _model(V, cd, mode)
        got.append([m.generate(text, z, N, text_mask=mask, return_logprobs=True, **kw) for kw in calls])
    for a, b in zip(*got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))


@pytest.mark.parametrize("V,cd", SHAPES[:2], ids=SHAPE_IDS[:2])
def test_without_the_flag_the_step_runs_as_before(V, cd, monkeypatch):
    """The fixed row count of the generic step's BLAS projections (mtts/decode.py
    _proj_blas) belongs to the flag: generate() and a session without it call
    every projection with rows = 0, the path that pads nothing and slices
    nothing, and so does decode_step; with it, with BLAS_ROWS.  The fused
    bf16 step never gets there."""
    from mtts import decode
    seen = []
    real = decode._proj_blas

    def spy(x, w, b=None, act=None, rows=0):
        seen.append(rows)
        return real(x, w, b, act, rows)

    monkeypatch.setattr(decode, "_proj_blas", spy)
    m = _model(V, cd, "eager")
    text, z, mask = _conds()

    def rows_of(run):
        del seen[:]
        run()
        return set(seen)

    expect = (lambda *r: set()) if cd == torch.bfloat16 else (lambda *r: set(r))
    assert rows_of(lambda: m.generate(text, z, 3, text_mask=mask)) == expect(0)
    assert rows_of(lambda: m.generate(text, z, 3, text_mask=mask, return_logprobs=True)) == expect(decode.BLAS_ROWS)
    assert rows_of(lambda: m.generate(text, z, 3, text_mask=mask, temperature=[1.0] * B)) == expect(0)
    with torch.no_grad():
        tok = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        assert rows_of(lambda: m.decode_step(tok, text, z, [None] * 2, 0, text_mask=mask)) == expect(0)
    for flag in (False, True):
        ses = m.open_session(2, KEYS, repetition_window=WINDOW, logprobs=flag)
        ses.admit(0, **_request(V, 0, 4))
        assert rows_of(lambda: ses.run(2)) == expect(decode.BLAS_ROWS if flag else 0)
    # rows = 0 is the old expression: the very tensor the GEMM returned, nothing padded, nothing sliced
    x, w = torch.randn(3, 8, device=DEV), torch.randn(5, 8, device=DEV)
    assert torch.equal(real(x, w), x @ w.t()) and real(x, w).shape == (3, 5) and real(x, w)._base is None
    assert real(x, w, rows=32).shape == (3, 5) and real(x, w, rows=32)._base is not None


# ---- sessions -------------------------------------------------------------------
def _request(V, i, cap, **over):
    g = torch.Generator().manual_seed(50 + i)
    r = dict(text_hidden=torch.randn(LENS[i % 3], D, generator=g).to(DEV), z_style=torch.randn(DS, generator=g).to(DEV),
             max_new_tokens=cap, temperature=MIXED["temperature"][i % 3], top_k=MIXED["top_k"][i % 3],
             top_p=MIXED["top_p"][i % 3], seed=1000 + 7 * i, repetition_penalty=PENALTY[i % 3],
             logit_bias=_bias(V, 30 + i) if i % 2 else None)
    r.update(over)
    return r


def _solo(ses, slot, req):
    ses.admit(slot, **req)
    pt = req.get("prompt_tokens")
    ses.run(req["max_new_tokens"] - (1 if pt is not None and pt.shape[-1] > 1 else 0))
    assert slot in ses.poll()
    return ses.take(slot, return_logprobs=True)


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("V,cd", SHAPES, ids=SHAPE_IDS)
def test_session_column_is_the_reference_on_the_logits_of_its_step(V, cd, mode):
    m = _model(V, cd, mode)
    slots = 3
    ses = m.open_session(slots, KEYS, repetition_window=WINDOW, logprobs=True)
    assert ses.captures == (1 if mode == "graph" else 0) and ses.g["lp_hist"].shape == (slots, 256)
    reqs = [_request(V, 0, 20), _request(V, 1, 26), _request(V, 2, 12)]
    penalty = [r["repetition_penalty"] for r in reqs]
    bias = np.zeros((slots, V), dtype=np.float32)
    for s, r in enumerate(reqs):
        if r["logit_bias"] is not None:
            bias[s] = r["logit_bias"].cpu().numpy()
    ses.admit(0, **reqs[0])
    ses.admit(1, **reqs[1])
    checked = 0
    for t in range(28):
        if t == 5:
            ses.admit(2, **reqs[2])                         # five replays late: the slots sit at different columns
        draw, fin = ses.g["draw"].cpu().tolist(), ses.finished.cpu().tolist()
        hist = ses.g["hist"].cpu().numpy()
        before = ses.g["lp_hist"].clone()
        ses.run(1)
        lg = ses.logits.float().cpu().numpy()
        tok = ses.eng.tok_buf[:, 0].cpu().numpy()
        after = ses.g["lp_hist"]
        touched = torch.zeros_like(after, dtype=torch.bool)
        for s in range(slots):
            if fin[s]:
                continue                                    # idle or done at entry: nothing of the row may move
            col = draw[s]
            touched[s, col] = True
            ref = LP.logprob_ref(lg[s:s + 1], [tok[s]], bias=bias[s:s + 1], penalty=penalty[s:s + 1], window=WINDOW,
                                 history=hist[s:s + 1], col=[col], draw=[col])[0]
            err = abs(float(after[s, col]) - ref)
            assert err <= LP.lp_bound(V, LP.threads_of(V), ref), (t, s, col, float(after[s, col]), ref)
            checked += 1
        assert torch.equal(_bits(after[~touched]), _bits(before[~touched])), t
    assert checked == 20 + 26 + 12 and sorted(ses.poll()) == [0, 1, 2]
    for s, r in enumerate(reqs):
        toks, lps = ses.take(s, return_logprobs=True)
        assert toks.shape == lps.shape == (r["max_new_tokens"],) and lps.dtype == torch.float32
        assert bool((lps < 0).all())
    assert ses.captures == (1 if mode == "graph" else 0)    # an open session never captures again


def _alone(m, V, req, cap, rows=1, row=0):
    """generate() on the request in row `row` of `rows` (the other rows: empty conditioning, greedy)."""
    S = req["text_hidden"].shape[0]
    text = torch.zeros(rows, KEYS, D, device=DEV)
    text[row, :S] = req["text_hidden"]
    mask = torch.zeros(rows, KEYS, dtype=torch.bool, device=DEV)
    mask[:, 0] = True
    mask[row, :S] = True
    z = torch.zeros(rows, DS, device=DEV)
    z[row] = req["z_style"]
    bias = torch.zeros(rows, V, device=DEV)
    bias[row] = req["logit_bias"]
    put = lambda v, fill: [fill] * row + [v] + [fill] * (rows - row - 1)  # noqa: E731
    toks, lens, lps = m.generate(text, z, cap, text_mask=mask, temperature=put(req["temperature"], 0.0),
                                 top_k=put(req["top_k"], 0), top_p=put(req["top_p"], 1.0), seed=put(req["seed"], 0),
                                 repetition_penalty=put(req["repetition_penalty"], 1.0), repetition_window=WINDOW,
                                 logit_bias=bias, return_logprobs=True)
    assert lens.tolist() == [cap] * rows
    return toks[row], lps[row]


@pytest.mark.parametrize("V,cd", SHAPES, ids=SHAPE_IDS)
def test_a_request_gives_the_same_bits_in_any_slot_and_company(V, cd):
    m = _model(V, cd)
    cap = 24
    req = _request(V, 1, cap)                               # sampled, filtered, penalised, biased
    ses = m.open_session(20, KEYS, repetition_window=WINDOW, logprobs=True)
    want_t, want_lp = _solo(ses, 1, req)                    # slot 1 of an otherwise idle session
    assert want_t.shape == want_lp.shape == (cap,) and len(torch.unique(want_lp)) > cap // 2
    ses.admit(16, **_request(V, 0, 100))
    ses.admit(18, **_request(V, 2, 80))
    ses.run(7)                                              # the neighbours are 7 tokens in
    t, lp = _solo(ses, 17, req)
    assert torch.equal(t, want_t) and torch.equal(_bits(lp), _bits(want_lp))
    other_t, other_lp = _solo(ses, 17, _request(V, 3, 15, seed=5))          # another request through the slot ...
    assert other_t.shape == other_lp.shape == (15,)
    t, lp = _solo(ses, 17, req)                             # ... and right after it left
    assert torch.equal(t, want_t) and torch.equal(_bits(lp), _bits(want_lp))
    assert ses.captures == 1
    # generate() with as many rows as the session has slots, the request in row 17: the same step
    # launches over the same row count, so the same logits -- and the same bits -- in both dtypes
    t, lp = _alone(m, V, req, cap, rows=20, row=17)
    assert torch.equal(t, want_t) and torch.equal(_bits(lp), _bits(want_lp))


@pytest.mark.parametrize("V,cd", SHAPES, ids=SHAPE_IDS)
def test_session_logprobs_equal_generate_on_the_request_alone(V, cd):
    """The request in slot 17 of a 20-slot session against generate() at batch
    1, bit for bit, on the fused bf16 step (row-wise HIP kernels) and on the
    fp32 generic step, whose BLAS projections run at one fixed row count when
    log-probabilities are asked for (mtts/decode.py _proj_blas, step_fn) so
    that their rounding cannot depend on how many rows share the step.  Before that the request's fp32 LOGITS differed
    between 20 rows and 1 row by 2.0e-6 (V 10) / 4.8e-6 (V 300) and its
    log-probabilities with them, by 14 / 67 ulp, while the tokens agreed."""
    m = _model(V, cd)
    cap = 24
    req = _request(V, 1, cap)
    ses = m.open_session(20, KEYS, repetition_window=WINDOW, logprobs=True)
    want_t, want_lp = _solo(ses, 17, req)
    t, lp = _alone(m, V, req, cap)
    print(f"V {V} {cd}: session vs generate() at batch 1, max |d logprob| {float((lp - want_lp).abs().max()):.3e}, "
          f"max bit distance {int((_bits(lp).long() - _bits(want_lp).long()).abs().max())}")
    assert torch.equal(t, want_t)
    assert torch.equal(_bits(lp), _bits(want_lp))


def test_take_and_the_queue():
    V = 10
    m = _model(V, torch.bfloat16)
    req = _request(V, 1, 9)
    ses = m.open_session(2, KEYS, repetition_window=WINDOW)
    assert "lp_hist" not in ses.g
    ses.admit(0, **req)
    ses.run(9)
    with pytest.raises(ValueError, match="logprobs"):
        ses.take(0, return_logprobs=True)
    toks = ses.take(0)                                      # the refusal changed nothing
    assert toks.shape == (9,)
    # the queue: a fourth element, the requests' log-probabilities in request order
    reqs = [_request(V, i, cap) for i, cap in enumerate((12, 5, 9, 7))]
    out = m.generate_requests(reqs, slots=2, max_keys=KEYS, check_every=4, repetition_window=WINDOW,
                              return_logprobs=True)
    plain = m.generate_requests(reqs, slots=2, max_keys=KEYS, check_every=4, repetition_window=WINDOW)
    assert len(out) == 4 and len(plain) == 3 and out[1:3] == plain[1:3]
    assert all(torch.equal(a, b) for a, b in zip(out[0], plain[0]))
    lp_ses = m.open_session(2, KEYS, repetition_window=WINDOW, logprobs=True)
    for i, r in enumerate(reqs):
        t, lp = _solo(lp_ses, i % 2, r)
        assert torch.equal(t, out[0][i]) and torch.equal(_bits(lp), _bits(out[3][i])), i
    assert m.generate_requests([], slots=2, return_logprobs=True) == ([], [], 0, [])
