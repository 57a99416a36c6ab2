"""CPU-side checks of the per-row token sampler's boundary and of its float64
reference (tests/sample_rows_ref.py): MttsSampleRowsArgs as the C compiler
lays it out against the ctypes mirror, the exported symbol and the unchanged
ABI version, the reference on its own (the distribution of one row's stream,
its independence of row index and batch size, a hand-worked penalty case) and
ops.row_seeds against the numpy mix64."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

import sample_ref as SR
import sample_rows_ref as RR

HEADER = os.path.join(ROOT, "include", "mtts.h")
LOGITS = np.array([2, 1, .5, 0, -.5, -1, .3, 1.5, -2, .1])
ROWS = 20000
CHI2_BOUND = 33.7   # chi-square, 9 degrees of freedom, p = 1e-4 (as tests/test_sample_cpu.py)


def test_sample_rows_args_layout_symbol_and_abi():
    from mtts import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(MttsSampleRowsArgs));', 'printf("wmax %d\\n", MTTS_SAMPLE_WINDOW_MAX);']
    for fname, _ in _lib.SampleRowsArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(MttsSampleRowsArgs, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        exe = os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        field, val = line.split()
        if field == "wmax":
            assert int(val) == 256
            continue
        got = ctypes.sizeof(_lib.SampleRowsArgs) if field == "size" else getattr(_lib.SampleRowsArgs, field).offset
        assert got == int(val), f"SampleRowsArgs.{field}: ctypes {got} != C {val}"
        seen += 1
    assert seen == len(_lib.SampleRowsArgs._fields_) + 1
    lib = _lib.lib()
    assert hasattr(lib, "mtts_sample_tokens_rows") and "mtts_sample_tokens_rows" in _lib.exported_symbols()
    assert "mtts_sample_tokens" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


def _chi2(tokens, p):
    n = len(tokens)
    obs = np.bincount(tokens, minlength=len(p)).astype(np.float64)
    return float((((obs - n * p) ** 2) / (n * p)).sum())


def _ctl(rows, **kw):
    d = dict(temperature=[1.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[99] * rows, draw=[0] * rows)
    d.update(kw)
    return d


def test_reference_row_stream_draws_from_softmax():
    # one row's stream: the same seed, draw = 0 .. ROWS - 1
    p = np.exp(LOGITS) / np.exp(LOGITS).sum()
    tok, _ = RR.sample_rows_ref(np.tile(LOGITS, (ROWS, 1)), **_ctl(ROWS, draw=list(range(ROWS))))
    chi = _chi2(tok, p)
    print(f"chi-square of {ROWS} draws of one stream vs softmax, 9 dof: {chi:.2f}")
    assert chi < CHI2_BOUND, chi
    # another seed is another stream: the two agree about sum p^2 (21 %) of the time
    other, _ = RR.sample_rows_ref(np.tile(LOGITS, (ROWS, 1)), **_ctl(ROWS, seed=[100] * ROWS, draw=list(range(ROWS))))
    agree = float((other == tok).mean())
    print(f"seed 100 agrees with seed 99 on {agree:.3f} of the draws (sum p^2 = {(p * p).sum():.3f})")
    assert abs(agree - (p * p).sum()) < 0.03, agree


def test_reference_stream_ignores_row_index_and_batch_size():
    rng = np.random.RandomState(0)
    x = (3 * rng.randn(5, 37)).astype(np.float32)
    seeds, draws = [7, -3, 2 ** 62, 7, 11], [0, 5, 9, 1, 300]
    kw = dict(temperature=[0.8, 1.0, 1.3, 0.8, 0.5], top_k=[0, 5, 0, 3, 0], top_p=[1.0, 0.9, 0.7, 1.0, 0.95])
    tok, acc = RR.sample_rows_ref(x, seed=seeds, draw=draws, **kw)
    perm = [3, 0, 4, 2, 1]
    tok_p, acc_p = RR.sample_rows_ref(x[perm], seed=[seeds[i] for i in perm], draw=[draws[i] for i in perm],
                                      **{k: [v[i] for i in perm] for k, v in kw.items()})
    assert tok_p.tolist() == tok[perm].tolist() and acc_p == [acc[i] for i in perm]
    for r in range(5):
        t1, a1 = RR.sample_rows_ref(x[r:r + 1], seed=seeds[r:r + 1], draw=draws[r:r + 1],
                                    **{k: v[r:r + 1] for k, v in kw.items()})
        assert int(t1[0]) == int(tok[r]) and a1[0] == acc[r]
    # the noise itself: a function of (seed, draw, v)
    assert np.array_equal(RR.row_gumbel(7, 3, 37), RR.row_gumbel(7 + (1 << 64), 3, 37))
    assert not np.array_equal(RR.row_gumbel(7, 3, 37), RR.row_gumbel(7, 4, 37))


def test_reference_penalty_hand_worked():
    V = 8
    x = np.array([2.0, -1.0, 0.0, -np.inf, 3.0, 1.5, -0.5, 4.0], dtype=np.float32)
    hist = np.array([7, 0, 0, 1, 2, 3, -1, V, 5, 6], dtype=np.int64)
    # col 9, window 8: columns 1..8 hold {0, 0, 1, 2, 3, -1, V, 5}; -1 and V are ignored, 0 counts once
    ids = RR.window_ids(hist, 9, 100, 8, V)
    assert ids == {0, 1, 2, 3, 5}
    y = RR.penalise(x, ids, 2.0)
    #        2 / 2  -1 * 2  0    -inf     untouched  1.5 / 2  untouched
    assert y.tolist() == [1.0, -2.0, 0.0, -np.inf, 3.0, 0.75, -0.5, 4.0] and y.dtype == np.float32
    # clipped by the number of tokens the row has drawn: columns 7..8 -> {5}
    assert RR.window_ids(hist, 9, 2, 8, V) == {5}
    # clipped by the column: only column 0 lies before column 1 -> {7}
    assert RR.window_ids(hist, 1, 100, 8, V) == {7}
    assert RR.window_ids(hist, 0, 100, 8, V) == set() and RR.window_ids(hist, 9, 0, 8, V) == set()
    assert RR.window_ids(hist, 9, 100, 0, V) == set()
    # a penalty below one favours repeats: positive multiplied up, negative shrunk; fp32 rounding
    z = RR.penalise(x, {0, 1}, 0.3)
    assert z[0] == np.float32(2.0) / np.float32(0.3) and z[1] == np.float32(-1.0) * np.float32(0.3)
    # no-ops
    for theta in (1.0, 0.0, -2.0, float("nan"), float("inf")):
        assert np.array_equal(RR.penalise(x, ids, theta), x), theta
    # through the sampler: greedy sees the penalised row (4.0 / 8 < 3.0)
    kw = dict(temperature=[0.0], top_k=[0], top_p=[1.0], seed=[1], draw=[9], history=hist[None], col=9)
    assert RR.sample_rows_ref(x[None], **kw)[0].tolist() == [7]
    hist2 = hist.copy()
    hist2[8] = 7
    kw["history"] = hist2[None]
    assert RR.sample_rows_ref(x[None], penalty=[8.0], window=8, **kw)[0].tolist() == [4]
    assert RR.sample_rows_ref(x[None], penalty=[8.0], window=0, **kw)[0].tolist() == [7]
    assert RR.sample_rows_ref(x[None], penalty=[float("nan")], window=8, **kw)[0].tolist() == [7]


def test_reference_effective_rules_match_scalar_reference():
    # with the controls off, or equal in every row, the per-row reference keeps sample_ref's kept sets
    rng = np.random.RandomState(1)
    x = (3 * rng.randn(4, 50)).astype(np.float32)
    tok, _ = RR.sample_rows_ref(x, temperature=[0.0, -1.0, float("nan"), 0.0], top_k=[0] * 4, top_p=[1.0] * 4,
                                seed=[1] * 4, draw=[0] * 4)
    assert tok.tolist() == np.argmax(x, 1).tolist()
    a = RR.sample_rows_ref(x, temperature=[0.9] * 4, top_k=[0, -5, 50, 53], top_p=[1.0, 0.0, 1.5, float("nan")],
                           seed=[5] * 4, draw=[2] * 4)
    b = RR.sample_rows_ref(x, temperature=[0.9] * 4, top_k=[0] * 4, top_p=[1.0] * 4, seed=[5] * 4, draw=[2] * 4)
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1]


def test_row_seeds_against_numpy_mix64():
    from mtts import ops
    for seed in (0, 7, -1, 2 ** 63 - 1, -2 ** 63, 123456789012345):
        got = ops.row_seeds(seed, 9)
        r = np.arange(1, 10, dtype=np.uint64)
        want = SR.mix64(np.uint64(seed % (1 << 64)) + r * SR.GOLDEN).astype(np.int64)
        assert got == want.tolist(), seed
        assert all(-2 ** 63 <= s < 2 ** 63 for s in got) and len(set(got)) == 9
    assert ops.row_seeds(7, 3) == ops.row_seeds(7, 9)[:3] and ops.row_seeds(7, 0) == []
