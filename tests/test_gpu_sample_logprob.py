"""The sampler's token log-probabilities (ops.sample_tokens* with logprob /
logprob_history; csrc/sample.hip, the kLogprob instantiations) against the
float64 reference (tests/sample_logprob_ref.py), in all three forms, f32 and
bf16 logits, across the one-wave boundary (V = 256 / 257) and the first row
that is not staged in LDS (V = 4097), 1 / 3 / 32 rows, every launch mixing
greedy, top-k, top-p, penalised (windows 0 / 8 / 256, duplicate ids), biased,
finished, all -inf and +inf rows.  Per launch:
  1. tokens and every piece of bookkeeping equal the same call without the
     outputs: the feature does not move a draw;
  2. every row's value is within lp_bound of the reference evaluated at the
     kernel's own token, NaN where the maximum is not finite, 0.0 for a row
     finished at entry -- no row is skipped;
  3. the history column is placed by the form's rule and a sentinel filling
     the rest of the buffer is untouched (slot form: a finished row's column
     too);
  4. a second launch gives the same bits;
and the same row gives the same bits at row 0 of 1 and at row 17 of 32.
The largest err / bound per V goes to profiles/sample_logprobs_parity.txt."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import sample_logprob_ref as LP

pytestmark = pytest.mark.gpu
DEV = "cuda"
HC = 270            # history columns: above the largest column used (256 + 5)
SENTINEL = -7.5
KINDS = ("greedy", "topk1", "topp", "pen", "bias", "finished", "allneg", "posinf", "plain")
FORMS = ("scalar", "rows", "slots")
SCALAR_CTL = ((0.0, 0, 1.0), (1.0, 1, 1.0), (0.8, 0, 0.9), (1.3, 0, 1.0))
PARITY = os.path.join(ROOT, "profiles", "sample_logprobs_parity.txt")
_worst = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _case(form, dtype, V, rows, launch, kinds=None):
    """One launch's inputs on the host: logits, bias, controls, history and
    bookkeeping, the rows' kinds cycling with the launch index."""
    rng = np.random.RandomState(1000 * V + launch)
    g = torch.Generator().manual_seed(1000 * V + launch)
    kinds = [KINDS[(launch + r) % len(KINDS)] for r in range(rows)] if kinds is None else kinds
    w = (0, 8, 256)[launch % 3]
    logits = (3 * torch.randn(rows, V, generator=g)).to(dtype)
    bias = np.zeros((rows, V), dtype=np.float32)
    for r, k in enumerate(kinds):
        if k == "bias":
            bias[r] = rng.randn(V).astype(np.float32)
            bias[r, rng.rand(V) < 0.3] = -np.inf
            bias[r, rng.randint(V)] = 0.5
        elif k == "allneg":
            logits[r] = float("-inf")
        elif k == "posinf":
            logits[r, rng.randint(V)] = float("inf")
    draws = [(0, 1, w + 5, 3, max(w, 2))[(launch + r) % 5] for r in range(rows)]
    hist = rng.randint(0, min(V, 24), size=(rows, HC)).astype(np.int64)     # a small range: duplicates are the rule
    c = dict(form=form, V=V, rows=rows, w=w, kinds=kinds, logits=logits, bias=bias, hist=hist, draws=draws,
             fin=[1 if k == "finished" else 0 for k in kinds], length=list(draws), pad=1 if V > 1 else 0,
             col=w + 2, step0=5)
    if form == "scalar":
        c["ctl"] = SCALAR_CTL[launch % len(SCALAR_CTL)]
    else:
        per = dict(greedy=(0.0, 0, 1.0, 1.0), topk1=(1.0, 1, 1.0, 1.0), topp=(0.8, 0, 0.9, 1.0),
                   pen=(1.0, 0, 1.0, 1.3), plain=(1.3, 0, 1.0, 1.3))
        pick = [per.get(k, (1.0, 0, 1.0, 1.0)) for k in kinds]
        c["ctl"] = dict(temperature=[p[0] for p in pick], top_k=[p[1] for p in pick], top_p=[p[2] for p in pick],
                        penalty=[p[3] for p in pick], seed=rng.randint(-2 ** 62, 2 ** 62, size=rows).tolist())
    return c


def _launch(c, outputs, only=None):
    """The case on fresh device buffers.  Returns everything the launch wrote."""
    from mtts import ops
    rows, form = c["rows"], c["form"]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    st = dict(hist=torch.from_numpy(c["hist"]).to(DEV), fin=i32(c["fin"]),
              length=torch.tensor(c["length"], dtype=torch.int64, device=DEV), unf=i32([-1]),
              pos=i32([d + 3 for d in c["draws"]]), step=i32([c["col"] + c["step0"]]))
    kw = dict(logit_bias=torch.from_numpy(c["bias"]).to(DEV), history=st["hist"], pad_id=c["pad"], finished=st["fin"],
              length=st["length"], unfinished=st["unf"], pos=st["pos"], step=st["step"], advance=True)
    if outputs:
        st["lp"] = torch.full((rows,), SENTINEL, device=DEV)
        st["lph"] = torch.full((rows, HC), SENTINEL, device=DEV)
        if only != "history":
            kw["logprob"] = st["lp"]
        if only != "vector":
            kw["logprob_history"] = st["lph"]
    lg = c["logits"].to(DEV)
    if form == "scalar":
        T, k, p = c["ctl"]
        st["tok"] = ops.sample_tokens(lg, temperature=T, top_k=k, top_p=p, seed=1234, step0=c["step0"], **kw)
    else:
        ctl = c["ctl"]
        st["draw"] = i32(c["draws"])
        d = dict(temperature=torch.tensor(ctl["temperature"], device=DEV), top_k=i32(ctl["top_k"]),
                 top_p=torch.tensor(ctl["top_p"], device=DEV), penalty=torch.tensor(ctl["penalty"], device=DEV),
                 seed=torch.tensor(ctl["seed"], dtype=torch.int64, device=DEV), draw=st["draw"], window=c["w"])
        if form == "rows":
            st["tok"] = ops.sample_tokens_rows(lg, step0=c["step0"], **d, **kw)
        else:
            st["tok"] = ops.sample_tokens_slots(lg, **d, **kw)
    return st


def _columns(c):
    return c["draws"] if c["form"] == "slots" else [c["col"]] * c["rows"]


def _reference(c, tokens):
    lg = c["logits"].float().numpy()
    if c["form"] == "scalar":
        return LP.logprob_ref(lg, tokens, bias=c["bias"])
    return LP.logprob_ref(lg, tokens, bias=c["bias"], penalty=c["ctl"]["penalty"], window=c["w"], history=c["hist"],
                          col=_columns(c), draw=c["draws"])


def _check(c, where):
    """Assertions 1-4 on one case; returns the largest err / bound."""
    V, rows, form = c["V"], c["rows"], c["form"]
    plain = _launch(c, outputs=False)
    got = _launch(c, outputs=True)
    for k in plain:                                         # 1: nothing else moved
        assert torch.equal(plain[k], got[k]), f"{where}: {k} differs from the call without the outputs"
    tok = got["tok"].cpu().numpy()
    lp, lph = got["lp"].cpu().numpy(), got["lph"].cpu().numpy()
    ref = _reference(c, tok)
    cols = _columns(c)
    expect_hist = np.full((rows, HC), SENTINEL, dtype=np.float32)
    worst = 0.0
    for r, kind in enumerate(c["kinds"]):                   # 2: every row
        what = f"{where} row {r} ({kind}, token {tok[r]}, column {cols[r]})"
        if kind == "finished":
            assert lp[r] == 0.0 and tok[r] == c["pad"], what
            if form != "slots":
                expect_hist[r, cols[r]] = 0.0
            continue
        if kind in ("allneg", "posinf"):
            assert np.isnan(ref[r]) and np.isnan(lp[r]), f"{what}: {lp[r]} (reference {ref[r]})"
        else:
            bound = LP.lp_bound(V, LP.threads_of(V), ref[r])
            err = abs(float(lp[r]) - ref[r])
            assert np.isfinite(ref[r]) and err <= bound, f"{what}: {lp[r]!r} vs {ref[r]!r}, err {err:.3e} > {bound:.3e}"
            worst = max(worst, err / bound)
        expect_hist[r, cols[r]] = lp[r]
    # 3: the column by the form's rule, the sentinel everywhere else (NaN compares by bits)
    assert np.array_equal(lph.view(np.int32), expect_hist.view(np.int32)), f"{where}: logprob history misplaced"
    again = _launch(c, outputs=True)                        # 4
    assert torch.equal(_bits(again["lp"]), _bits(got["lp"])) and torch.equal(_bits(again["lph"]), _bits(got["lph"])), \
        f"{where}: a second launch gave other bits"
    return worst


def _record(V, worst):
    _worst[V] = worst
    try:
        with open(PARITY, "w") as f:
            f.write("largest |logprob - float64 reference| / lp_bound over the grid of tests/test_gpu_sample_logprob.py\n"
                    "(three forms x f32 / bf16 x 1 / 3 / 32 rows; bound = 2^-23 (ceil(V / threads) + 16 + ln V + 2 |ref|))\n")
            for v in sorted(_worst):
                f.write(f"V {v:5d}  threads {LP.threads_of(v):3d}  err / bound {_worst[v]:.3f}\n")
    except OSError:
        pass


@pytest.mark.parametrize("V", [1, 10, 256, 257, 1024, 4096, 4097])
def test_grid_against_reference(V):
    launch, worst, seen = 0, 0.0, set()
    for form in FORMS:
        for dtype in (torch.float32, torch.bfloat16):
            for rows in (1, 3, 32):
                c = _case(form, dtype, V, rows, launch)
                worst = max(worst, _check(c, f"{form} {dtype} V {V} rows {rows} w {c['w']} launch {launch}"))
                seen |= {(form, k) for k in c["kinds"]}
                launch += 1
    assert seen == {(f, k) for f in FORMS for k in KINDS}   # every kind of row ran in every form
    print(f"V {V}: largest err / bound {worst:.3f}")
    _record(V, worst)


@pytest.mark.parametrize("V", [10, 256, 257, 4097])
def test_a_row_gives_the_same_bits_wherever_it_sits(V):
    for form in FORMS:
        for dtype in (torch.float32, torch.bfloat16):
            for kind in ("pen", "bias", "topp"):
                big = _case(form, dtype, V, 32, 4, kinds=[KINDS[r % len(KINDS)] for r in range(17)] + [kind]
                            + ["plain"] * 14)
                if form == "scalar":
                    big["ctl"] = (0.0, 0, 1.0)              # the scalar form's stream depends on the row: greedy
                one = dict(big, rows=1, kinds=[kind], logits=big["logits"][17:18].clone(), bias=big["bias"][17:18],
                           hist=big["hist"][17:18], draws=big["draws"][17:18], fin=[0], length=big["length"][17:18])
                if form != "scalar":
                    one["ctl"] = {k: v[17:18] for k, v in big["ctl"].items()}
                a, b = _launch(big, outputs=True), _launch(one, outputs=True)
                col = _columns(big)[17]
                where = f"{form} {dtype} V {V} {kind}"
                assert int(a["tok"][17]) == int(b["tok"][0]), where
                assert torch.equal(_bits(a["lp"][17:18]), _bits(b["lp"])), where
                assert torch.equal(_bits(a["lph"][17, col:col + 1]), _bits(b["lph"][0, col:col + 1])), where
                assert torch.isfinite(b["lp"]).all() and float(b["lp"]) <= 0.0, where


def test_either_output_alone_and_without_a_token_history():
    from mtts import ops
    for form in FORMS:
        c = _case(form, torch.float32, 300, 3, 0, kinds=["plain", "finished", "pen"])
        both = _launch(c, outputs=True)
        vec = _launch(c, outputs=True, only="vector")
        his = _launch(c, outputs=True, only="history")
        assert torch.equal(_bits(vec["lp"]), _bits(both["lp"])) and bool((vec["lph"] == SENTINEL).all()), form
        assert torch.equal(_bits(his["lph"]), _bits(both["lph"])) and bool((his["lp"] == SENTINEL).all()), form
        for st in (vec, his):
            assert torch.equal(st["tok"], both["tok"]) and torch.equal(st["hist"], both["hist"]), form
    # no token history: the log-probability history's own width bounds the column
    lg = torch.randn(2, 40, device=DEV)
    for cols, hit in ((4, True), (3, False)):
        lph = torch.full((2, cols), SENTINEL, device=DEV)
        tok = ops.sample_tokens(lg, temperature=0.0, seed=0, step=3, logprob_history=lph)
        want = torch.log_softmax(lg.double(), -1).gather(1, tok[:, None])[:, 0]
        if hit:
            assert bool((lph[:, :3] == SENTINEL).all())
            for r in range(2):
                assert abs(float(lph[r, 3]) - float(want[r])) <= LP.lp_bound(40, 64, float(want[r]))
        else:
            assert bool((lph == SENTINEL).all())


def test_wrong_outputs_are_refused_by_name_before_any_launch():
    from mtts import _lib, ops
    rows, V = 4, 16
    lg = torch.zeros(rows, V, device=DEV)
    hist = torch.zeros(rows, 8, dtype=torch.int64, device=DEV)
    per = dict(temperature=torch.ones(rows, device=DEV), top_k=torch.zeros(rows, dtype=torch.int32, device=DEV),
               top_p=torch.ones(rows, device=DEV), seed=torch.zeros(rows, dtype=torch.int64, device=DEV),
               draw=torch.zeros(rows, dtype=torch.int32, device=DEV))
    calls = ((ops.sample_tokens, dict(seed=0, step=0)), (ops.sample_tokens_rows, dict(step=0, **per)),
             (ops.sample_tokens_slots, per))
    bad_vec = (torch.zeros(rows, device=DEV, dtype=torch.float64), torch.zeros(rows + 1, device=DEV),
               torch.zeros(rows, 2, device=DEV)[:, 0], torch.zeros(rows), [0.0] * rows)
    bad_hist = (torch.zeros(rows, 8, device=DEV, dtype=torch.float64), torch.zeros(rows, 7, device=DEV),
                torch.zeros(rows + 1, 8, device=DEV), torch.zeros(8, rows, device=DEV).t(), torch.zeros(rows, 8),
                torch.zeros(rows * 8, device=DEV), torch.zeros(1, 8, device=DEV).expand(rows, 8))
    for fn, kw in calls:
        for t in bad_vec:
            with pytest.raises(ValueError, match=r"logprob must"):
                fn(lg, history=hist, logprob=t, **kw)
        for t in bad_hist:
            with pytest.raises(ValueError, match=r"logprob_history must"):
                fn(lg, history=hist, logprob_history=t, **kw)
    assert per["draw"].cpu().tolist() == [0] * rows         # nothing ran
    # the entry point's own checks (a caller that bypasses the binding)
    a = _lib.SampleArgs()
    out = torch.zeros(rows, dtype=torch.int64, device=DEV)
    a.rows, a.vocab, a.dtype, a.ld, a.logits, a.tokens, a.tok_stride = rows, V, _lib.F32, V, lg.data_ptr(), \
        out.data_ptr(), 1
    a.temperature, a.top_p, a.eos_id = 1.0, 1.0, -1
    with pytest.raises(RuntimeError, match="sample_tokens_lp: no logprob output"):
        _lib.call("mtts_sample_tokens_lp", a, _lib.SampleLogprobOut())
    a.hist_cols = 8
    lph = torch.zeros(rows, 4, device=DEV)
    with pytest.raises(RuntimeError, match="sample_tokens_lp: bad logprob history shape"):
        _lib.call("mtts_sample_tokens_lp", a, _lib.SampleLogprobOut(logprob_history=lph.data_ptr(), lp_ld=4))
