"""float64 numpy reference of the token sampler (include/mtts.h, MttsSampleArgs;
csrc/sample.hip), shared by tests/test_sample_cpu.py (which checks the
reference on its own, against the distributions it must draw from) and the
GPU tests (which check the kernel against it).

x_v = logit_v + bias_v, the sum taken in fp32 (the format of both inputs, and
what the kernel compares), NaN -> -inf; everything after that in float64.

Besides the exact token the reference returns, per row, an ACCEPTANCE SET: the
tokens a correct fp32 implementation may return.  It is the union, over two
kept sets, of the tokens whose score x_v / T + g_v is within SCORE_TOL of the
best score: the kept set with every token whose S_> = sum_{p_w > p_v} p_w lies
within V * 2^-22 of top_p counted in, and the one with all of them counted out
(twice the worst-case fp32 rounding of a V-term sum); SCORE_TOL = 1e-4 covers
the fp32 error of x / T + g (|score| < 32: ulp 4e-6; logf good to 2 ulp).
Top-k is a count of exact comparisons and has no tolerance.
"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
SCORE_TOL = 1e-4


def mix64(z):
    """splitmix64's finalizer on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def gumbel(seed, step, rows, V):
    """g (rows, V) float64: -log(-log(u)), u = ((h >> 40) + 0.5) * 2^-24,
    h = mix64(seed + c * golden), c = (step * rows + row) * V + v (mod 2^64)."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    v = np.arange(V, dtype=np.uint64)[None, :]
    s = np.full((1, 1), int(step) % (1 << 64), dtype=np.uint64)
    sd = np.full((1, 1), int(seed) % (1 << 64), dtype=np.uint64)
    c = (s * np.uint64(rows) + r) * np.uint64(V) + v
    h = mix64(sd + c * GOLDEN)
    u = ((h >> np.uint64(40)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def inputs(logits, bias=None):
    """x (rows, V) float64 from fp32-representable logits and an optional fp32
    bias (V,) or (rows, V)."""
    x = np.asarray(logits, dtype=np.float32)
    if bias is not None:
        with np.errstate(invalid="ignore"):
            x = x + np.asarray(bias, dtype=np.float32)
    x = x.astype(np.float64)
    x[np.isnan(x)] = -np.inf
    return x


def kept_sets(x, T, top_k, top_p):
    """x (V,) float64.  Returns (exact, counted_in, counted_out) boolean masks
    of the kept set (see the module docstring)."""
    V = x.shape[0]
    keep = x > -np.inf
    if top_k > 0:
        asc = np.sort(x)
        greater = V - np.searchsorted(asc, x, side="right")     # #{w : x_w > x_v}
        keep &= greater < top_k
    if not keep.any() or top_p >= 1.0:
        return keep, keep, keep
    m = x[keep].max()
    with np.errstate(invalid="ignore"):
        p = np.where(keep, np.exp((x - m) / T), 0.0)
    p = p / p.sum()
    desc = np.sort(p)[::-1]
    csum = np.concatenate([[0.0], np.cumsum(desc)])
    n_greater = V - np.searchsorted(desc[::-1], p, side="right")   # #{w : p_w > p_v}
    S = csum[n_greater]                                            # sum of those
    tol = V * 2.0 ** -22
    top = keep & (n_greater == 0)                                  # the most likely token always survives
    return keep & (S < top_p), keep & (S < top_p + tol), (keep & (S < top_p - tol)) | top


def sample_ref(logits, *, temperature=1.0, top_k=0, top_p=1.0, bias=None, seed=0, step=0, pad_id=0):
    """tokens (rows,) int64 and the per-row acceptance sets (a list of sets)."""
    x = inputs(logits, bias)
    rows, V = x.shape
    tokens = np.empty(rows, dtype=np.int64)
    accept = []
    g = gumbel(seed, step, rows, V) if temperature > 0 else None
    for r in range(rows):
        xr = x[r]
        if not (xr > -np.inf).any():
            tokens[r] = pad_id
            accept.append({pad_id})
            continue
        if temperature == 0:
            tokens[r] = int(np.argmax(xr))                          # first index on ties
            accept.append({int(tokens[r])})
            continue
        exact, k_in, k_out = kept_sets(xr, temperature, top_k, top_p)
        score = xr / temperature + g[r]
        tokens[r] = int(np.argmax(np.where(exact, score, -np.inf)))
        acc = set()
        for keep in (k_in, k_out):
            s = np.where(keep, score, -np.inf)
            acc |= set(np.nonzero(s >= s.max() - SCORE_TOL)[0].tolist())
        accept.append(acc)
    return tokens, accept


def ambiguous_share(accept):
    """Share of rows whose acceptance set has more than one member."""
    return sum(len(a) > 1 for a in accept) / max(len(accept), 1)
