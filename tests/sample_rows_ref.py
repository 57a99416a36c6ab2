"""float64 numpy reference of the per-row token sampler (include/mtts.h,
MttsSampleRowsArgs; csrc/sample.hip), shared by tests/test_sample_rows_cpu.py
(the reference on its own) and the GPU tests (the kernel and generate()
against it).  It is tests/sample_ref.py with

  * the controls per row and the header's effective rules: !(T > 0) is greedy,
    top_k <= 0 or >= V is off, top_p outside (0, 1) is off, a penalty t with
    !(t > 0), t == 1 or t == inf is off (T, top_p and t as the fp32 values the
    kernel reads);
  * the row's own stream: h = mix64(seed_r + (draw_r * V + v) * golden), a
    function of (seed_r, draw_r, v) only;
  * the repetition penalty, computed in np.float32 like the bias sum (top-k
    compares exact keys, so the penalised value must be the kernel's bit for
    bit): with n = min(window, draw_r, col), each distinct id of
    history[r, col - n .. col) inside [0, V) has x_v / t for x_v > 0, else
    x_v * t.

Tokens and acceptance sets mean what they mean in sample_ref.sample_ref.
"""
import numpy as np

import sample_ref as SR


def row_gumbel(seed, draw, V):
    """g (V,) float64 of one row: the stream of (seed, draw)."""
    v = np.arange(V, dtype=np.uint64)
    c = np.uint64(int(draw) % (1 << 64)) * np.uint64(V) + v
    h = SR.mix64(np.uint64(int(seed) % (1 << 64)) + c * SR.GOLDEN)
    u = ((h >> np.uint64(40)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def window_ids(hist_row, col, draw, window, V):
    """The set S of one row: distinct in-range ids among its last
    min(window, draw, col) history columns before `col`."""
    n = min(int(window), int(draw), int(col))
    if n <= 0 or hist_row is None:
        return set()
    cols = range(col - n, min(col, len(hist_row)))      # columns the buffer does not have are skipped
    return {int(hist_row[c]) for c in cols if 0 <= int(hist_row[c]) < V}


def penalty_on(theta):
    t = np.float32(theta)
    return bool(t > 0) and t != np.float32(1) and bool(np.isfinite(t))


def penalise(x32, ids, theta):
    """x32 (V,) float32 (NaN already -inf) with the penalty applied once to
    every id in `ids`; correctly rounded fp32 division / multiplication."""
    x = np.array(x32, dtype=np.float32)
    if not penalty_on(theta):
        return x
    t = np.float32(theta)
    with np.errstate(over="ignore", under="ignore"):
        for v in ids:
            x[v] = x[v] / t if x[v] > 0 else x[v] * t
    return x


def sample_rows_ref(logits, *, temperature, top_k, top_p, seed, draw, penalty=None, window=0, history=None, col=0,
                    bias=None, pad_id=0, finished=None):
    """tokens (rows,) int64 and the per-row acceptance sets.  The per-row
    arguments are sequences of `rows` values; history (rows, n) integers and
    `col` the column this draw is written to (*step - step0)."""
    x_all = SR.inputs(logits, bias)
    rows, V = x_all.shape
    tokens = np.empty(rows, dtype=np.int64)
    accept = []
    for r in range(rows):
        if finished is not None and finished[r]:
            tokens[r] = pad_id
            accept.append({pad_id})
            continue
        xr = x_all[r].astype(np.float32)
        if penalty is not None:
            xr = penalise(xr, window_ids(None if history is None else history[r], col, draw[r], window, V), penalty[r])
        xr = xr.astype(np.float64)
        T = float(np.float32(temperature[r]))
        k = int(top_k[r])
        k = 0 if k <= 0 or k >= V else k
        p = float(np.float32(top_p[r]))
        p = p if 0.0 < p < 1.0 else 1.0
        if not (xr > -np.inf).any():
            tokens[r] = pad_id
            accept.append({pad_id})
            continue
        if not T > 0 or xr.max() == np.inf:
            tokens[r] = int(np.argmax(xr))                      # first index on ties
            accept.append({int(tokens[r])})
            continue
        exact, k_in, k_out = SR.kept_sets(xr, T, k, p)
        score = xr / T + row_gumbel(seed[r], draw[r], V)
        tokens[r] = int(np.argmax(np.where(exact, score, -np.inf)))
        acc = set()
        for keep in (k_in, k_out):
            s = np.where(keep, score, -np.inf)
            acc |= set(np.nonzero(s >= s.max() - SR.SCORE_TOL)[0].tolist())
        accept.append(acc)
    return tokens, accept
