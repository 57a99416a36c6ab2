"""CPU-side checks of the sampler's token log-probabilities: the float64
reference (tests/sample_logprob_ref.py) on its own -- against
torch.log_softmax, its NaN rules, biased and penalised rows -- the bound
lp_bound against a float32 restatement of the kernel's summation order (and
two mutants that must exceed it), MttsSampleLogprobOut as the C compiler lays
it out, the three added symbols under the unchanged ABI version, and the
argument checks of the _lp entry points without a GPU.

The checks' table follows tests/test_sample_checks_cpu.py: host addresses
stand for every pointer and every row MUST fail a check, since a call that
passed them all would launch a kernel on those addresses."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT

import sample_logprob_ref as LP
import sample_rows_ref as RR

HEADER = os.path.join(ROOT, "include", "mtts.h")
GRID_V = (1, 2, 10, 64, 256, 257, 1024, 4096, 4097, 20000)
GRID_ROWS = 200
SCALES = (0.01, 0.3, 1.0, 3.0, 10.0, 30.0)


# ---- the reference ------------------------------------------------------------
def test_reference_is_log_softmax_of_the_processed_row():
    rng = np.random.RandomState(0)
    for V in (1, 2, 10, 257, 4097):
        x = (4 * rng.randn(6, V)).astype(np.float32)
        bias = (rng.randn(6, V)).astype(np.float32)
        bias[rng.rand(6, V) < 0.2] = -np.inf
        bias[:, 0] = 0.0                                    # every row keeps a finite candidate
        tok = [int(np.argmax(r)) for r in x + bias]
        tok[-1] = 0
        got = LP.logprob_ref(x, tok, bias=bias)
        want = torch.log_softmax(torch.from_numpy((x + bias).astype(np.float64)), dim=-1).numpy()
        for r in range(6):
            assert abs(got[r] - want[r, tok[r]]) <= 1e-12 * (1 + abs(want[r, tok[r]])), (V, r)
    # a one-entry vocabulary is certain; a uniform row gives -ln V
    assert LP.logprob_ref(np.array([[3.5]], dtype=np.float32), [0])[0] == 0.0
    assert abs(LP.logprob_ref(np.zeros((1, 1000), dtype=np.float32), [7])[0] + np.log(1000)) < 1e-12
    # the sampling controls do not enter: the function does not even take them
    with pytest.raises(TypeError):
        LP.logprob_ref(x, tok, temperature=[0.5] * 6)


def test_reference_nan_rules():
    inf = np.inf
    x = np.array([[1.0, -inf, np.nan, 2.0],      # NaN counts as -inf: finite maximum
                  [-inf, -inf, np.nan, -inf],    # no finite candidate
                  [1.0, inf, 0.0, 0.0],          # a +inf logit
                  [-inf, 0.5, -inf, -inf]], dtype=np.float32)
    got = LP.logprob_ref(x, [3, 0, 1, 1])
    assert abs(got[0] - (2.0 - np.log(np.exp(1.0) + np.exp(2.0)))) < 1e-12
    assert np.isnan(got[1]) and np.isnan(got[2])
    assert got[3] == 0.0
    # a bias can cause either: -inf everywhere, or +inf somewhere
    z = np.zeros((2, 4), dtype=np.float32)
    b = np.array([[-inf] * 4, [0, inf, 0, 0]], dtype=np.float32)
    assert np.isnan(LP.logprob_ref(z, [0, 1], bias=b)).all()


def test_reference_sees_bias_and_penalty_like_the_token_reference():
    V = 8
    x = np.array([[2.0, -1.0, 0.0, -np.inf, 3.0, 1.5, -0.5, 4.0]], dtype=np.float32)
    hist = np.array([[7, 0, 0, 1, 2, 3, -1, V, 5, 6]], dtype=np.int64)
    # the hand-worked window of test_sample_rows_cpu.py: col 9, window 8 -> ids {0, 1, 2, 3, 5}, theta 2
    y = np.array([1.0, -2.0, 0.0, -np.inf, 3.0, 0.75, -0.5, 4.0])
    for t in (7, 0, 5):
        got = LP.logprob_ref(x, [t], penalty=[2.0], window=8, history=hist, col=9, draw=[100])[0]
        assert abs(got - (y[t] - np.log(np.exp(y).sum()))) < 1e-12, t
    # the slot form's column is the row's own draw count
    a = LP.logprob_ref(x, [7], penalty=[2.0], window=8, history=hist, col=[9], draw=[9])[0]
    assert a == LP.logprob_ref(x, [7], penalty=[2.0], window=8, history=hist, col=9, draw=[100])[0]
    # a switched-off penalty, an empty window and no penalty at all agree
    plain = LP.logprob_ref(x, [7])[0]
    assert LP.logprob_ref(x, [7], penalty=[1.0], window=8, history=hist, col=9, draw=[9])[0] == plain
    assert LP.logprob_ref(x, [7], penalty=[2.0], window=0, history=hist, col=9, draw=[9])[0] == plain
    assert a != plain
    # the processed row is the token reference's, bit for bit
    p = LP.processed_rows(x, penalty=[2.0], window=8, history=hist, col=9, draw=[100])
    assert p.dtype == np.float32
    assert np.array_equal(p[0], RR.penalise(x[0], RR.window_ids(hist[0], 9, 100, 8, V), 2.0))


# ---- the bound ------------------------------------------------------------------
def _grid_rows(V, rng):
    """GRID_ROWS processed rows: every logit scale, -inf entries, a penalised
    share (what matters to the sum is only the values)."""
    x = rng.randn(GRID_ROWS, V).astype(np.float32)
    x *= np.array(SCALES, dtype=np.float32)[np.arange(GRID_ROWS) % len(SCALES)][:, None]
    x[rng.rand(GRID_ROWS, V) < 0.1] = -np.inf
    x[:, rng.randint(V)] = np.float32(0.25)                 # a finite candidate in every row
    return x


def _worst(V, **hooks):
    rng = np.random.RandomState(1000 + V)
    x = _grid_rows(V, rng)
    worst = 0.0
    for r in range(GRID_ROWS):
        finite = np.nonzero(np.isfinite(x[r]))[0]
        t = int(finite[rng.randint(len(finite))]) if r % 2 else int(np.argmax(x[r]))
        ref = LP.logprob_of(x[r], t)
        got = float(LP.kernel_order_f32(x[r], t, **hooks))
        worst = max(worst, abs(got - ref) / LP.lp_bound(V, LP.threads_of(V), ref))
    return worst


@pytest.mark.parametrize("V", GRID_V)
def test_kernel_order_in_float32_stays_within_the_bound(V):
    w = _worst(V)
    print(f"V {V}: worst err / bound of the float32 restatement = {w:.3f}")
    assert w <= 1.0, w


def test_bound_formula():
    assert LP.threads_of(256) == 64 and LP.threads_of(257) == 256
    assert LP.lp_bound(256, 64, -2.0) == 2.0 ** -23 * (4 + 16 + np.log(256) + 4.0)
    assert LP.lp_bound(4097, 256, 0.0) == 2.0 ** -23 * (17 + 16 + np.log(4097))
    assert LP.lp_bound(1, 64, 0.0) == 2.0 ** -23 * 17


def test_mutants_exceed_the_bound():
    # the criterion can fail: a log-probability at the sampling temperature, and one that skips the penalty
    T = np.float32(0.7)
    for V in (10, 257, 4097):
        tempered = _worst(V, exp_arg=lambda x, m: (x - m) / T, out_of=lambda x, m, t: (x[t] - m) / T)
        assert tempered > 10.0, (V, tempered)
    rng = np.random.RandomState(7)
    V = 300
    x = (3 * rng.randn(1, V)).astype(np.float32)
    hist = rng.randint(0, V, size=(1, 40)).astype(np.int64)
    t = int(hist[0, 30])                                    # a penalised token
    ref = LP.logprob_ref(x, [t], penalty=[1.3], window=16, history=hist, col=32, draw=[32])[0]
    skipped = float(LP.kernel_order_f32(x[0], t))           # the row without its penalty
    kept = float(LP.kernel_order_f32(LP.processed_rows(x, penalty=[1.3], window=16, history=hist, col=32,
                                                       draw=[32])[0], t))
    bound = LP.lp_bound(V, 256, ref)
    assert abs(kept - ref) <= bound < abs(skipped - ref) / 10


# ---- the boundary -----------------------------------------------------------------
def test_logprob_out_layout_symbols_and_unchanged_structs():
    from mtts import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(MttsSampleLogprobOut));',
             'printf("scalar %zu\\n", sizeof(MttsSampleArgs));', 'printf("rows %zu\\n", sizeof(MttsSampleRowsArgs));',
             'printf("abi %d\\n", MTTS_ABI_VERSION);']
    for fname, _ in _lib.SampleLogprobOut._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(MttsSampleLogprobOut, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        exe = os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert [f for f, _ in _lib.SampleLogprobOut._fields_] == ["logprob", "logprob_history", "lp_ld"]
    assert got.pop("size") == C.sizeof(_lib.SampleLogprobOut) == 24
    # the structs the existing entry points take are what they were
    assert got.pop("scalar") == C.sizeof(_lib.SampleArgs) == 160
    assert got.pop("rows") == C.sizeof(_lib.SampleRowsArgs) == 200
    assert got.pop("abi") == 15
    for fname, _ in _lib.SampleLogprobOut._fields_:
        assert got.pop(fname) == getattr(_lib.SampleLogprobOut, fname).offset, fname
    assert not got
    lib = _lib.lib()
    for sym in ("mtts_sample_tokens_lp", "mtts_sample_tokens_rows_lp", "mtts_sample_tokens_slots_lp"):
        assert hasattr(lib, sym) and sym in _lib.exported_symbols(), sym
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


def test_ops_take_both_outputs_and_default_to_none():
    import inspect

    from mtts import ops
    for fn in (ops.sample_tokens, ops.sample_tokens_rows, ops.sample_tokens_slots):
        prm = inspect.signature(fn).parameters
        assert prm["logprob"].default is None and prm["logprob_history"].default is None


# ---- the _lp entry points' checks -------------------------------------------------
EINVAL = -22
ROWS, VOCAB = 4, 16
_BUF = (C.c_int64 * 64)()          # a host buffer whose address stands for every pointer; never dereferenced
PTR = C.addressof(_BUF)
SCALAR, PER_ROW, SLOTS = "sample_tokens_lp", "sample_tokens_rows_lp", "sample_tokens_slots_lp"
ARRAYS = ("temperature", "top_k", "top_p", "seed", "draw")
GOOD_LP = dict(logprob=PTR, logprob_history=PTR, lp_ld=8)
NO_STRUCT = "no struct"


def _base(entry):
    from mtts import _lib
    io = dict(rows=ROWS, vocab=VOCAB, dtype=_lib.F32, ld=VOCAB, logits=PTR, tokens=PTR, tok_stride=1, step=PTR,
              eos_id=-1, pad_id=0)
    if entry == SCALAR:
        return _lib.SampleArgs(temperature=1.0, top_k=0, top_p=1.0, seed=PTR, **io)
    return _lib.SampleRowsArgs(window=0, **{k: PTR for k in ARRAYS}, **io)


def _table():
    """(entry point, fields overwritten in the valid base struct, the output
    struct -- a dict, or NO_STRUCT for a NULL pointer --, the message)."""
    hist = dict(history=PTR, hist_cols=8, hist_ld=8)
    t = []
    for n in (SCALAR, PER_ROW, SLOTS):
        t += [
            # the two new checks, on an otherwise valid call
            (n, {}, NO_STRUCT, f"{n}: no logprob output"),
            (n, {}, dict(logprob=None, logprob_history=None, lp_ld=8), f"{n}: no logprob output"),
            (n, hist, dict(logprob=None, logprob_history=None, lp_ld=8), f"{n}: no logprob output"),
            (n, hist, dict(logprob=None, logprob_history=PTR, lp_ld=7), f"{n}: bad logprob history shape"),
            (n, hist, dict(logprob=PTR, logprob_history=PTR, lp_ld=0), f"{n}: bad logprob history shape"),
            (n, hist, dict(logprob=PTR, logprob_history=PTR, lp_ld=-1), f"{n}: bad logprob history shape"),
            (n, dict(hist_cols=8), dict(logprob_history=PTR, lp_ld=4), f"{n}: bad logprob history shape"),
            # their order: the missing output before the shape
            (n, hist, dict(logprob=None, logprob_history=None, lp_ld=-1), f"{n}: no logprob output"),
            # an existing fault is still reported first, with its message
            (n, None, GOOD_LP, f"{n}: null pointer"),
            (n, None, NO_STRUCT, f"{n}: null pointer"),
            (n, dict(logits=None), NO_STRUCT, f"{n}: null pointer"),
            (n, dict(dtype=2), NO_STRUCT, f"{n}: dtype must be f32 or bf16"),
            (n, dict(rows=0), GOOD_LP, f"{n}: rows=0 vocab={VOCAB} out of range"),
            (n, dict(ld=VOCAB - 1), dict(logprob=None, logprob_history=None, lp_ld=0), f"{n}: row stride below vocab"),
            (n, dict(pad_id=VOCAB), NO_STRUCT, f"{n}: pad_id={VOCAB} / eos_id=-1 outside the vocabulary"),
            (n, dict(history=PTR, hist_cols=8, hist_ld=4), dict(logprob_history=PTR, lp_ld=4),
             f"{n}: bad history shape"),
            (n, dict(unfinished=PTR), NO_STRUCT, f"{n}: unfinished needs finished"),
        ]
    t += [
        (SCALAR, dict(temperature=-1.0), NO_STRUCT, f"{SCALAR}: temperature=-1.000000 must be >= 0"),
        (SCALAR, dict(top_p=1.5), GOOD_LP, f"{SCALAR}: top_p=1.500000 must be in (0, 1]"),
    ]
    for n in (SCALAR, PER_ROW):
        t += [
            (n, dict(advance=1, step=None), NO_STRUCT, f"{n}: advance needs step"),
            (n, dict(pos_rows=-1), dict(logprob=None, logprob_history=None, lp_ld=0),
             f"{n}: pos_rows=-1 must be >= 0"),
        ]
    for n in (PER_ROW, SLOTS):
        t += [
            (n, dict(draw=None), NO_STRUCT, f"{n}: temperature, top_k, top_p, seed and draw are required"),
            (n, dict(window=257), NO_STRUCT, f"{n}: window=257 outside [0, 256]"),
            (n, dict(window=4), GOOD_LP, f"{n}: window=4 needs history"),
            (n, dict(max_length=PTR), NO_STRUCT, f"{n}: max_length needs finished and length"),
        ]
    t += [(SLOTS, dict(advance=1, pos=PTR, pos_rows=2), NO_STRUCT, f"{SLOTS}: pos_rows=2 must be 0 or rows={ROWS}")]
    return t


TABLE = _table()


def _fails_a_check(fields, lp):
    """A row may run only if it cannot reach the launch."""
    if fields is None or fields.keys() - {"history", "hist_cols", "hist_ld"}:
        return True                                          # an existing check's row: its message is asserted
    if lp == NO_STRUCT or (lp.get("logprob") is None and lp.get("logprob_history") is None):
        return True
    return lp.get("logprob_history") is not None and lp.get("lp_ld", 0) < fields.get("hist_cols", 0)


def run(entry, fields, lp):
    from mtts import _lib
    lib = _lib.lib()
    fn = getattr(lib, "mtts_" + entry)
    assert _fails_a_check(fields, lp), "a table row must make its call invalid"
    out = None if lp == NO_STRUCT else C.byref(_lib.SampleLogprobOut(**lp))
    if fields is None:
        rc = fn(None, out, None)
    else:
        a = _base(entry)
        for k, v in fields.items():
            assert any(k == f[0] for f in a._fields_), k
            setattr(a, k, v)
        rc = fn(C.byref(a), out, None)
    return rc, lib.mtts_last_error().decode()


def _id(row):
    entry, fields, lp, _ = row
    f = "null" if fields is None else ",".join(f"{k}={'ptr' if v == PTR else v}" for k, v in fields.items())
    o = lp if lp == NO_STRUCT else ",".join(f"{k}={'ptr' if v == PTR else v}" for k, v in lp.items())
    return f"{entry}-{f}-{o}"


@pytest.mark.parametrize("row", TABLE, ids=[_id(r) for r in TABLE])
def test_lp_entry_points_refuse_invalid_calls_with_their_message(row):
    entry, fields, lp, message = row
    rc, got = run(entry, fields, lp)
    assert rc == EINVAL
    assert got == message


def test_table_is_well_formed():
    assert len({_id(r) for r in TABLE}) == len(TABLE)
    for n in (SCALAR, PER_ROW, SLOTS):
        msgs = [r[3] for r in TABLE if r[0] == n]
        assert sum("no logprob output" in m for m in msgs) >= 3
        assert sum("bad logprob history shape" in m for m in msgs) >= 3
        assert sum("logprob" not in m for m in msgs) >= 9       # existing faults, reported first
