"""float64 numpy reference of the sampler's token log-probabilities
(include/mtts.h, MttsSampleLogprobOut; csrc/sample.hip), shared by
tests/test_sample_logprob_cpu.py (the reference on its own, and the bound
below against a float32 restatement of the kernel's summation order) and the
GPU tests (the kernel, generate() and the decode session against it).

The processed row x is built from the pieces the token references are built
from -- sample_ref.inputs (fp32 logit + fp32 bias, NaN -> -inf) and
sample_rows_ref.window_ids / penalise (the repetition penalty, correctly
rounded fp32) -- so it is the kernel's x bit for bit.  With m = max x and t the
emitted token,

    logprob = (x_t - m) - log(sum_v exp(x_v - m))       in float64,

NaN when m is not finite.  It does not look at temperature, top_k, top_p, the
seed or the draw count.

lp_bound(V, threads, ref) is what an fp32 implementation in the header's order may
differ by: 2^-23 * (ceil(V / threads) + 16 + ln V + 2 |ref|), threads = 64 for
V <= 256 and 256 above.  The fp32 sum of ceil(V / threads) positive terms per
thread plus the reduction tree (6 + 2 levels) and expf / logf good to 1 ulp
give a relative error of the sum of at most about (ceil(V / threads) + 16) *
2^-24, which is its absolute error after the logarithm; ln Z <= ln V is
rounded once, and x_t - m and the final difference are two roundings of
magnitude at most |ref| + ln V.
"""
import math

import numpy as np

import sample_ref as SR
import sample_rows_ref as RR


def threads_of(V):
    """Threads of the workgroup that takes a row of V entries."""
    return 64 if V <= 256 else 256


def processed_rows(logits, bias=None, penalty=None, window=0, history=None, col=0, draw=None):
    """x (rows, V) float32 as the sampler's load() makes it.  `col`: the
    history column of this draw, one int (scalar and per-row forms: *step -
    step0) or one per row (slot form: draw[r])."""
    x_all = SR.inputs(logits, bias)
    rows, V = x_all.shape
    out = np.empty((rows, V), dtype=np.float32)
    for r in range(rows):
        xr = x_all[r].astype(np.float32)
        if penalty is not None:
            c = int(col[r]) if np.ndim(col) else int(col)
            xr = RR.penalise(xr, RR.window_ids(None if history is None else history[r], c, draw[r], window, V),
                             penalty[r])
        out[r] = xr
    return out


def logprob_of(x, token):
    """One processed row x (V,) and its emitted token: the definition, float64."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    if not np.isfinite(m):
        return float("nan")
    with np.errstate(under="ignore"):
        return float((x[int(token)] - m) - np.log(np.exp(x - m).sum()))


def logprob_ref(logits, tokens, **processing):
    """(rows,) float64: logprob_of over processed_rows(logits, **processing)."""
    x = processed_rows(logits, **processing)
    return np.array([logprob_of(x[r], tokens[r]) for r in range(x.shape[0])], dtype=np.float64)


def lp_bound(V, threads, ref):
    return 2.0 ** -23 * (math.ceil(V / threads) + 16 + math.log(V) + 2 * abs(float(ref)))


def kernel_order_f32(x, token, threads=None, exp_arg=None, out_of=None):
    """The header's order restated in numpy float32 for one processed row:
    thread tid adds exp(x_v - m) for v = tid, tid + threads, ... in turn, a
    wave of 64 reduces by the xor butterfly (1, 2, 4, 8, 16, 32), four waves as
    (w0 + w1) + (w2 + w3).  exp_arg / out_of: hooks for the mutants of the CPU
    test (what is exponentiated; what the token's own term is)."""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[0]
    threads = threads_of(V) if threads is None else threads
    m = x.max()
    if not np.isfinite(m):
        return np.float32("nan")
    d = (x - m) if exp_arg is None else exp_arg(x, m)
    n = -(-V // threads)
    pad = np.full(n * threads, -np.inf, dtype=np.float32)
    pad[:V] = d
    with np.errstate(under="ignore"):
        e = np.exp(pad).reshape(n, threads)
    acc = np.zeros(threads, dtype=np.float32)
    for j in range(n):
        acc = acc + e[j]                      # fp32, ascending j (adding exp(-inf) = +0 changes nothing)
    lane = np.arange(threads)
    for o in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[lane ^ o]
    z = acc[0] if threads == 64 else (acc[0] + acc[64]) + (acc[128] + acc[192])
    xt = (x[int(token)] - m) if out_of is None else out_of(x, m, int(token))
    return np.float32(xt) - np.log(np.float32(z))
