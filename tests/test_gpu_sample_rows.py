"""The per-row token sampler (ops.sample_tokens_rows, csrc/sample.hip) against
its float64 reference (tests/sample_rows_ref.py) at the kernel's dispatch
edges -- one wave / four waves at V = 256, LDS-staged / re-read at V = 4096 --
with every launch mixing greedy, sampled, filtered and penalised rows; the
independence of a row's tokens from its place in the batch; a captured launch
following its per-row arrays; the end-of-sequence and length-cap bookkeeping;
and the window's bound check."""
import itertools

import numpy as np
import pytest
import torch

import sample_rows_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"

TEMPS = (0.0, 0.7, 1.0, 1.5)
TOPK = (0, 1, 5, "V+3")
TOPP = (1.0, 0.9, 0.5, 1e-6)
THETA = (1.0, 1.3, 0.8)
SETTINGS = list(itertools.product(TEMPS, TOPK, TOPP, THETA))
np.random.RandomState(5).shuffle(SETTINGS)
WINDOWS = (1, 4, 64)


def _settings(base, rows, V):
    pick = [SETTINGS[(base + r) % len(SETTINGS)] for r in range(rows)]
    return dict(temperature=[s[0] for s in pick], top_k=[V + 3 if s[1] == "V+3" else s[1] for s in pick],
                top_p=[s[2] for s in pick], penalty=[s[3] for s in pick])


def _dev(ctl):
    """The per-row lists as the device tensors the binding asks for."""
    dt = dict(temperature=torch.float32, top_k=torch.int32, top_p=torch.float32, seed=torch.int64,
              draw=torch.int32, penalty=torch.float32, max_length=torch.int64)
    return {k: torch.tensor(v, dtype=dt[k], device=DEV) for k, v in ctl.items()}


def _history(rng, rows, V, w, col, cols):
    """(rows, cols) random ids; the first half of the window before column
    `col` repeats its second half, so duplicates are the rule."""
    h = rng.randint(0, V, size=(rows, cols)).astype(np.int64)
    lo = max(col - w, 0)
    half = (col - lo) // 2
    if half:
        h[:, lo:lo + half] = h[:, col - half:col]
    return h


@pytest.mark.parametrize("V", [1, 10, 64, 65, 256, 257, 1024, 4096, 4097, 5000])
def test_grid_against_reference(V):
    from mtts import ops
    rng = np.random.RandomState(V)
    g = torch.Generator().manual_seed(V)
    launch, ambiguous, total = 0, 0, 0
    for dtype in (torch.float32, torch.bfloat16):
        for rows in ((1, 3, 33) if V < 1024 else (1, 3)):
            for w in WINDOWS:
                col = (w + 2, w // 2 + 1, w)[launch % 3]                # the window whole, and clipped by the column
                logits = (3 * torch.randn(rows, V, generator=g)).to(dtype)
                hist = _history(rng, rows, V, w, col, w + 8)
                draws = [(0, 1, w - 1, w, w + 5)[(launch + r) % 5] for r in range(rows)]
                ctl = _settings(7 * launch, rows, V)
                ctl.update(seed=rng.randint(-2 ** 62, 2 ** 62, size=rows).tolist(), draw=draws)
                want, acc = RR.sample_rows_ref(logits.float().numpy(), window=w, history=hist, col=col, **ctl)
                d = _dev(ctl)
                hist_d = torch.from_numpy(hist).to(DEV)
                tok = ops.sample_tokens_rows(logits.to(DEV), window=w, history=hist_d, step=col, **d)
                tok = tok.cpu().numpy()
                for r in range(rows):
                    assert int(tok[r]) in acc[r], (f"{dtype} rows {rows} w {w} col {col} row {r} "
                                                   f"{ {k: v[r] for k, v in ctl.items()} }: {tok[r]} not in "
                                                   f"{sorted(acc[r])} (reference {want[r]})")
                assert d["draw"].cpu().tolist() == [x + 1 for x in draws]
                assert hist_d[:, col].cpu().tolist() == tok.tolist()
                ambiguous += sum(len(a) > 1 for a in acc)
                total += rows
                launch += 1
    print(f"V {V}: {ambiguous} of {total} rows have an ambiguous acceptance set")
    assert ambiguous <= 0.01 * total, (ambiguous, total)


def _batch(V, rows=7, w=16, seed=3):
    rng = np.random.RandomState(seed + V)
    g = torch.Generator().manual_seed(seed + V)
    logits = 3 * torch.randn(rows, V, generator=g)
    col = w + 3
    hist = _history(rng, rows, V, w, col, col + 2)
    ctl = dict(temperature=[0.0, 0.7, 1.0, 1.5, 0.9, 1.0, 1.2], top_k=[0, 5, 0, 9, 0, 3, 0],
               top_p=[1.0, 0.9, 0.5, 1.0, 0.8, 1.0, 0.95], penalty=[1.3, 1.3, 0.8, 1.5, 1.0, 2.0, 1.3],
               seed=rng.randint(-2 ** 62, 2 ** 62, size=rows).tolist(), draw=[5, 16, 17, 40, 3, 16, 100])
    return logits, hist, col, ctl


@pytest.mark.parametrize("V", [64, 1027])
def test_tokens_do_not_depend_on_batch_composition(V):
    from mtts import ops
    rows, w = 7, 16
    logits, hist, col, ctl = _batch(V, rows, w)
    fin = [0, 0, 1, 0, 0, 1, 0]

    def run(order):
        d = _dev({k: [v[i] for i in order] for k, v in ctl.items()})
        f = torch.tensor([fin[i] for i in order], dtype=torch.int32, device=DEV)
        h = torch.from_numpy(hist[order]).to(DEV)
        tok = ops.sample_tokens_rows(logits[order].to(DEV), window=w, history=h, step=col, finished=f, pad_id=1, **d)
        return tok.cpu().tolist(), d["draw"].cpu().tolist()

    tok, drawn = run(list(range(rows)))
    assert drawn == [x + (0 if f else 1) for x, f in zip(ctl["draw"], fin)]
    assert [tok[r] for r in range(rows) if fin[r]] == [1, 1]
    rev = list(range(rows))[::-1]
    tok_r, drawn_r = run(rev)
    assert tok_r[::-1] == tok and drawn_r[::-1] == drawn
    for r in range(rows):
        t1, d1 = run([r])
        assert t1 == [tok[r]] and d1 == [drawn[r]], r
    _, acc = RR.sample_rows_ref(logits.numpy(), window=w, history=hist, col=col, finished=fin, pad_id=1, **ctl)
    assert all(tok[r] in acc[r] for r in range(rows))


def test_captured_launch_follows_its_per_row_arrays():
    from mtts import ops
    V, rows, w = 300, 5, 8
    g = torch.Generator().manual_seed(9)
    rng = np.random.RandomState(9)
    logits = (3 * torch.randn(rows, V, generator=g)).to(DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    hist = torch.zeros(rows, 16, dtype=torch.int64, device=DEV)
    out = torch.zeros(rows, dtype=torch.int64, device=DEV)
    d = _dev(dict(temperature=[1.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[0] * rows, draw=[0] * rows,
                  penalty=[1.0] * rows))

    def launch():
        ops.sample_tokens_rows(logits, window=w, history=hist, step=step, advance=True, out=out, **d)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        launch()
    step.zero_()
    hist.zero_()
    d["draw"].zero_()
    for i in range(3):
        ctl = dict(temperature=[(0.0, 0.7, 1.3)[(i + r) % 3] for r in range(rows)],
                   top_k=[(0, 4, 1)[(2 * i + r) % 3] for r in range(rows)],
                   top_p=[(1.0, 0.9, 0.5)[(i + 2 * r) % 3] for r in range(rows)],
                   seed=rng.randint(-2 ** 62, 2 ** 62, size=rows).tolist(),
                   penalty=[(1.5, 1.0, 0.8)[(i + r) % 3] for r in range(rows)])
        for k, v in _dev(ctl).items():
            d[k].copy_(v)
        before = hist.cpu().numpy()
        gr.replay()
        torch.cuda.synchronize()
        _, acc = RR.sample_rows_ref(logits.cpu().numpy(), window=w, history=before, col=i, draw=[i] * rows, **ctl)
        tok = out.cpu().tolist()
        assert all(tok[r] in acc[r] for r in range(rows)), (i, tok, acc)
        assert hist[:, i].cpu().tolist() == tok
        assert int(step) == i + 1 and d["draw"].cpu().tolist() == [i + 1] * rows


def test_bookkeeping_caps_eos_and_padding():
    from mtts import ops
    V, rows, eos, pad = 12, 6, 4, 2
    # greedy rows whose argmax is set by the bias: row 0 finished already, row 1 cap 1, row 2 cap and EOS together,
    # row 3 EOS before its cap, row 4 runs on, row 5 reaches its cap at the second draw
    first = [7, 9, eos, eos, 5, 6]
    logits = torch.zeros(rows, V, device=DEV)
    for r, t in enumerate(first):
        logits[r, t] = 5.0
    d = _dev(dict(temperature=[0.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[1] * rows, draw=[3] + [0] * 5,
                  max_length=[9, 1, 1, 5, 5, 2]))
    fin = torch.tensor([1, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    length = torch.tensor([3, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
    unf = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    hist = torch.full((rows, 4), -7, dtype=torch.int64, device=DEV)
    kw = dict(history=hist, step=step, advance=True, eos_id=eos, pad_id=pad, finished=fin, length=length,
              unfinished=unf, **d)
    tok = ops.sample_tokens_rows(logits, **kw)
    assert tok.cpu().tolist() == [pad, 9, eos, eos, 5, 6]
    assert fin.cpu().tolist() == [1, 1, 1, 1, 0, 0] and length.cpu().tolist() == [3, 1, 1, 1, 1, 1]
    assert d["draw"].cpu().tolist() == [3, 1, 1, 1, 1, 1] and int(unf) == 2 and int(step) == 1
    tok = ops.sample_tokens_rows(logits, **kw)
    assert tok.cpu().tolist() == [pad, pad, pad, pad, 5, 6]
    assert fin.cpu().tolist() == [1, 1, 1, 1, 0, 1] and length.cpu().tolist() == [3, 1, 1, 1, 2, 2]
    assert d["draw"].cpu().tolist() == [3, 1, 1, 1, 2, 2] and int(unf) == 1 and int(step) == 2
    tok = ops.sample_tokens_rows(logits, **kw)
    assert tok.cpu().tolist() == [pad, pad, pad, pad, 5, pad] and int(unf) == 1
    # the token at the cap is in the history and the next column is pad
    assert hist.cpu().tolist() == [[pad, pad, pad, -7], [9, pad, pad, -7], [eos, pad, pad, -7], [eos, pad, pad, -7],
                                   [5, 5, 5, -7], [6, 6, pad, -7]]
    assert length.cpu().tolist() == [3, 1, 1, 1, 3, 2] and d["draw"].cpu().tolist() == [3, 1, 1, 1, 3, 2]


@pytest.mark.parametrize("V", [40, 300, 4100])
def test_window_ids_outside_the_vocabulary_are_ignored(V):
    from mtts import ops
    rows, w, col = 4, 8, 9
    g = torch.Generator().manual_seed(V)
    rng = np.random.RandomState(V)
    logits = (3 * torch.randn(rows, V, generator=g)).to(DEV)
    good = rng.randint(0, V, size=(rows, 5)).astype(np.int64)
    hist = np.zeros((rows, 12), dtype=np.int64)
    hist[:, col - w:col] = np.stack([np.full(rows, -1), good[:, 0], np.full(rows, V), good[:, 1], good[:, 2],
                                     np.full(rows, 2 ** 40), good[:, 3], good[:, 4]], 1)
    short = np.zeros((rows, 12), dtype=np.int64)                       # the same window with those slots removed
    short[:, col - 5:col] = good
    ctl = dict(temperature=[0.0, 1.0, 0.8, 1.2], top_k=[0, 0, 6, 0], top_p=[1.0, 1.0, 1.0, 0.9],
               seed=[4, 5, 6, 7], draw=[20] * rows, penalty=[1.7] * rows)
    a = ops.sample_tokens_rows(logits, window=w, history=torch.from_numpy(hist).to(DEV), step=col, **_dev(ctl))
    b = ops.sample_tokens_rows(logits, window=5, history=torch.from_numpy(short).to(DEV), step=col, **_dev(ctl))
    assert torch.equal(a, b)
    _, acc = RR.sample_rows_ref(logits.cpu().numpy(), window=w, history=hist, col=col, **ctl)
    assert all(int(a[r]) in acc[r] for r in range(rows))
    off = ops.sample_tokens_rows(logits, window=0, history=torch.from_numpy(hist).to(DEV), step=col, **_dev(ctl))
    assert int(off[0]) == int(logits[0].argmax())


def test_host_validation_before_any_launch():
    from mtts import ops
    rows, V = 4, 16
    logits = torch.zeros(rows, V, device=DEV)
    good = _dev(dict(temperature=[1.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[0] * rows,
                     draw=[0] * rows, penalty=[1.0] * rows, max_length=[5] * rows))
    fin = torch.zeros(rows, dtype=torch.int32, device=DEV)
    length = torch.zeros(rows, dtype=torch.int64, device=DEV)
    hist = torch.zeros(rows, 8, dtype=torch.int64, device=DEV)
    base = dict(step=0, finished=fin, length=length, history=hist, window=4)
    wrong_dtype = dict(temperature=torch.float64, top_k=torch.int64, top_p=torch.float64, seed=torch.int32,
                       draw=torch.int64, penalty=torch.float64, max_length=torch.int32)
    for name in good:
        for bad in (good[name].to(wrong_dtype[name]),                                   # dtype
                    torch.zeros(rows + 1, dtype=good[name].dtype, device=DEV),          # length
                    torch.zeros(rows, 2, dtype=good[name].dtype, device=DEV)[:, 0],     # contiguity
                    good[name].cpu(), [0] * rows):                                      # device, not a tensor
            kw = dict(good)
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                ops.sample_tokens_rows(logits, **base, **kw)
    with pytest.raises(ValueError, match="window"):
        ops.sample_tokens_rows(logits, **dict(base, window=257), **good)
    with pytest.raises(ValueError, match="window"):
        ops.sample_tokens_rows(logits, **dict(base, history=None), **good)
    with pytest.raises(ValueError, match="max_length"):
        ops.sample_tokens_rows(logits, **dict(base, finished=None), **good)
    assert good["draw"].cpu().tolist() == [0] * rows and length.cpu().tolist() == [0] * rows   # nothing ran
    # the entry point's own checks (a caller that bypasses the binding)
    from mtts import _lib
    a = _lib.SampleRowsArgs()
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("mtts_sample_tokens_rows", a)
