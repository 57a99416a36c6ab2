"""The comparison that pins the kernels that open and close a training step:
the codec cross-entropy (csrc/loss.hip through mtts.loss.cross_entropy), the
embedding sum (mtts_embed_sum / mtts_embed_sum_at of csrc/regulate.hip through
mtts.embed) and the token-table gradient (mtts_embed_table_grad through
mtts.embed._table_grad).  Shared by tests/test_token_ref_cpu.py, which proves
this file on the CPU (the references against float64 autograd, the criterion
against the listed mutants), and tests/test_gpu_token_ops.py, which checks
the kernels against it.  Pure torch on the CPU.

`*_reference`: float64, from the values as stored (bf16 upcast, a strided
tensor read through its strides).
    cross-entropy: lse = m + log sum exp(x - m); row loss lse - x[t]; the mean
        over the rows whose target is not ignore_index (NaN when there is
        none, NaN when such a target lies outside [0, V)); dlogits =
        (softmax - onehot) gout / count, exactly 0 on ignored rows (also when
        every row is ignored and the loss is NaN); a row whose target is out
        of range has no one-hot term
    embedding sum: tok_w[tok] + q_w[qid] + pos_w[pid], an all-zero row where
        the token (or, for mtts_embed_sum_at, the position) is out of range;
        every table gradient a float64 index_add_
    table gradient: out[v] = sum of the rows of g whose id is v, ids outside
        [0, vocab) add nothing
`*_restatement`: the same in float32, in the kernel's order: the row sum of
exp over v = 0 .. V-1 in turn, 64-lane trees, 4 wave partials per 256-row
block, ce_sum_kernel's 256-way strided pass; (tok + pos) + quant rounded to
bf16 to nearest even; the table gradient per wave over rows r0 + w, r0 + w + 4,
..., the (w0 + w1) + (w2 + w3) combine, and the column sum over the blocks (4
waves of 8 running sums; the kernel takes 16 waves for few columns: the same
depth, not the same bits).  "<name>": the value as stored; "<name>32": before
the rounding to the storage dtype.

`check(got, ref, rest, dtype, name)`: ln_ref's criterion with ln_ref's two
constants.  Per tensor, every finite element:
    |got - ref| <= 8 max|rest32 - ref| + 1e-6 max|ref|
and a bf16 tensor is allowed one bf16 rounding of the element less.  Non-finite
values must sit where the reference has them (NaN on NaN, +-inf on the same
inf).  Where the reference is exactly 0 the output must be 0: an ignored
row's gradient, a table row no id names, a position row past L, a zero-filled
embedding row.  The tensors in EXACT (the count, and the embedding output,
which is two fp32 adds of exact operands and one rounding) are compared bit
for bit with the restatement's stored value.

CASES is the list both files run; make_inputs(name) builds a case's CPU
tensors from a generator seeded by the name.  MUTANTS are wrong restatements
`check` has to reject."""
import functools
import math
import types
import zlib

import torch
import torch.nn.functional as F

from ln_ref import BF16_ULP, FLOOR, RATIO

F32, BF16 = torch.float32, torch.bfloat16
NAN, INF = float("nan"), float("inf")
EXACT = ("count", "y")
IO_KEYS = ("dlogits", "y")           # the tensors stored in the I/O dtype of a case
CE_BLOCK = 256
EMB_BINS = 16                        # kEmbGradVMax: the register bins of embed_table_grad_kernel


def _tag(dt):
    return {F32: "f32", BF16: "bf16"}[dt]


NS = types.SimpleNamespace


# ------------------------------------------------------------------- the cases
def _ce(name, rows, V, io, ld=None, col0=0, ignore=-100, tgt="frac", kind="normal", gout=0.7):
    """rows x V logits in `io`, read at columns col0 .. col0 + V of rows of ld
    elements (NaN around them); tgt: "none" (no row ignored), "frac" (30 % of
    the targets are ignore), "block" (rows 256..511), "last", "all", "oor" (one
    target V, one -1); kind: "normal" (3 randn), "plus90", "minus90",
    "dominant" (one logit +60), "halfinf" (every other entry of row 3 -inf),
    "tinf" (row 5's target on a -inf entry), "coarse" (256 + 2 randn)."""
    return NS(op="ce", name=f"ce-{name}-{_tag(io)}", rows=rows, V=V, io=io, ld=ld or V, col0=col0, ignore=ignore,
              tgt=tgt, kind=kind, gout=gout)


def _emb(name, B, L, d, io, V=10, Q=4, P=40, layout="prologue", bad=False, QT=None, grads=True):
    """(B, L) tokens, tables of V / Q / P rows of width d, output in `io`;
    layout: "prologue" (positions 0..L-1, random quantizer ids), "codec"
    (QT = (Q, T): embed_codec_layout), "shuffled" (a permutation as pid, the
    index_add_ branch), "at" (per-row position ids, mtts_embed_sum_at);
    bad: one id V and one -1 ("at": also one position P); grads: whether the
    table gradients are part of the case."""
    return NS(op="emb", name=f"emb-{name}-{_tag(io)}", B=B, L=L, d=d, io=io, V=V, Q=Q, P=P, layout=layout, bad=bad,
              QT=QT, grads=grads and not bad and layout != "at")


def _tg(name, n, d, io, vocab=10, ids="uniform", pad=8):
    """g (n, d) in `io`, a view of (n, d + pad); ids: "uniform", "same",
    "ends" (0 and vocab - 1), "live" (from [0, 16)), "neg" (a few -1 / -7),
    "big" (a few 16, 17 and 2^40); "uniform" has one id equal to vocab, which
    only the HIP route skips: "valid" has none."""
    return NS(op="tg", name=f"tg-{name}-{_tag(io)}", n=n, d=d, io=io, vocab=vocab, ids=ids, pad=pad)


CE_ROWS = ((1, 3), (255, 10), (256, 10), (257, 10), (37, 1024), (5, 1), (70000, 3))
EMB_D = (4, 64, 256, 260, 512, 1024)
EMB_L = (1, 15, 16, 17, 33)
CODEC_QT = ((1, 7), (5, 64), (3, 129))
TG_D = (8, 256, 264, 512, 520, 1024)
TG_N = (1, 3, 4, 63, 64, 65, 16384, 16385, 16641, 20000)


def _cases():
    out = []
    for io in (F32, BF16):
        # cross-entropy
        out += [_ce(f"rows-{r}x{V}", r, V, io, tgt="frac" if r >= 37 else "none") for r, V in CE_ROWS]
        out += [_ce("strided-10", 300, 10, io, ld=22, col0=4), _ce("strided-64", 37, 64, io, ld=76, col0=4),
                _ce("strided-odd", 300, 10, io, ld=23, col0=3),      # bf16 rows on odd 2-byte boundaries
                _ce("ign-default", 300, 10, io), _ce("ign-block", 700, 10, io, ignore=0, tgt="block"),
                _ce("ign-last", 257, 10, io, ignore=0, tgt="last"), _ce("ign-all", 300, 10, io, ignore=0, tgt="all"),
                _ce("oor", 300, 10, io, tgt="oor"), _ce("gout-tensor", 300, 10, io, gout=1.3),
                _ce("codec", 100, 10, io, ld=22, col0=4, ignore=0, tgt="frac")]
        out += [_ce(f"num-{k}", 300, 10, io, kind=k) for k in ("plus90", "minus90", "dominant", "halfinf", "tinf",
                                                               "coarse")]
        out += [_ce(f"graph-{k}", 300, 10, io, ignore=0, tgt=t) for k, t in (("a", "frac"), ("b", "last"),
                                                                             ("c", "block"))]
        # embedding sum
        out += [_emb(f"d-{d}", 2, 17, d, io) for d in EMB_D]
        out += [_emb(f"L-{L}", 2, L, 64, io) for L in EMB_L]
        out += [_emb("tokstride", 3, 17, 64, io), _emb("quant2d", 3, 17, 64, io),
                _emb("quant70", 2, 33, 64, io, Q=70), _emb("vocab40", 2, 33, 64, io, V=40),
                _emb("vocab300", 2, 33, 64, io, V=300), _emb("shuffled", 2, 17, 64, io, layout="shuffled")]
        out += [_emb(f"codec-{Q}x{T}", 2, Q * T, 64, io, Q=Q, P=Q * T + 3, layout="codec", QT=(Q, T))
                for Q, T in CODEC_QT]
        out += [_emb(f"bad-{d}", 2, 17, d, io, bad=True) for d in (64, 260)]
        out += [_emb("at", 4, 5, 64, io, Q=1, P=50, layout="at"),
                _emb("at-bad", 4, 5, 64, io, Q=1, P=50, layout="at", bad=True)]
        # token-table gradient
        out += [_tg(f"d-{d}", 1000, d, io) for d in TG_D]
        out += [_tg(f"n-{n}", n, 64, io) for n in TG_N]
        out += [_tg("ids-same", 1000, 64, io, ids="same"), _tg("ids-ends", 1000, 64, io, ids="ends"),
                _tg("vocab16", 1000, 64, io, vocab=16), _tg("vocab1", 1000, 64, io, vocab=1),
                _tg("ids-live", 1000, 64, io, ids="live"), _tg("ids-neg", 1000, 64, io, ids="neg"),
                _tg("ids-big", 1000, 64, io, ids="big")]
        out += [_tg(f"route-v{v}", 1000, 64, io, vocab=v, ids="valid") for v in (17, 64, 65)]
        out.append(_tg("route-stride", 1000, 64, io, ids="valid", pad=4))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(prefix):
    return [c.name for c in CASES if c.name.startswith(prefix)]


def emb_grad_blocks(n):
    """csrc/regulate.hip: (rows per block, blocks) of embed_table_grad_kernel."""
    r = max(64, (n + 255) // 256)
    r = (r + 3) // 4 * 4
    return r, (n + r - 1) // r


def table_route(c):
    """The route mtts.embed._table_grad takes for a tg case."""
    if c.vocab <= EMB_BINS and (c.d + c.pad) % 8 == 0 and c.d % 8 == 0:
        return "hip"
    return "onehot" if c.vocab <= 64 else "index_add"


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)
    if c.op == "ce":
        rows, V = c.rows, c.V
        x = rn(rows, V) * 3
        lo = 1 if c.ignore == 0 else 0          # ignore_index 0: the other rows' targets are 1 .. V-1
        t = ri(lo, V, rows)
        if c.tgt == "frac":
            t[torch.rand(rows, generator=g) < 0.3] = c.ignore
        elif c.tgt == "block":
            t[256:512] = c.ignore
        elif c.tgt == "last":
            t[-1] = c.ignore
        elif c.tgt == "all":
            t[:] = c.ignore
        elif c.tgt == "oor":
            t[torch.rand(rows, generator=g) < 0.3] = c.ignore
            t[17], t[280] = V, -1
        if c.kind == "plus90":
            x = x + 90.0
        elif c.kind == "minus90":
            x = x - 90.0
        elif c.kind == "dominant":
            x[torch.arange(rows), ri(0, V, rows)] += 60.0
        elif c.kind == "halfinf":
            x[3, 0::2] = -INF
            t[3] = 1
        elif c.kind == "tinf":
            t[5] = 2
            x[5, 2] = -INF
        elif c.kind == "coarse":
            x = 256.0 + 2.0 * rn(rows, V)
        buf = torch.full((rows, c.ld), NAN).to(c.io)
        buf[:, c.col0:c.col0 + V] = x.to(c.io)
        return NS(case=c, buf=buf, x=buf[:, c.col0:c.col0 + V], t=t, ignore=c.ignore, gout=c.gout)
    if c.op == "emb":
        B, L, d = c.B, c.L, c.d
        tok = ri(0, c.V, B, L)
        tw, qw, pw = rn(c.V, d), rn(c.Q, d), rn(c.P, d)
        if c.layout == "codec":
            Q, T = c.QT
            qid = torch.arange(Q).repeat_interleave(T)
            pid = torch.arange(T).repeat(Q)
        elif c.layout == "at":
            qid = torch.zeros(L, dtype=torch.long)
            pid = ri(0, c.P, B, L)
            pid[0, 0], pid[B - 1, L - 1] = 0, c.P - 1
        else:
            qid = ri(0, c.Q, L)
            pid = torch.randperm(L, generator=g) if c.layout == "shuffled" else torch.arange(L)
        if c.bad:
            tok[0, L // 2], tok[B - 1, L - 1] = c.V, -1
            if c.layout == "at":
                pid[1, 1] = c.P
        return NS(case=c, tok=tok, qid=qid.to(torch.int32), pid=pid.to(torch.int32), tw=tw, qw=qw, pw=pw,
                  dy=rn(B, L, d).to(c.io))
    n, d = c.n, c.d
    hi = EMB_BINS if c.ids == "live" else c.vocab
    ids = ri(0, hi, n)
    if c.ids == "same":
        ids[:] = min(3, c.vocab - 1)
    elif c.ids == "ends":
        ids = ri(0, 2, n) * (c.vocab - 1)
    elif c.ids == "neg":
        ids[5], ids[500], ids[-1] = -1, -7, -1
    elif c.ids == "big":
        ids[5], ids[500], ids[-1] = 16, 17, 2 ** 40
    elif n > 3 and c.ids == "uniform":
        ids[3] = c.vocab          # out of the table: the forward flags it, the gradient skips it
    buf = torch.full((n, d + c.pad), NAN).to(c.io)
    buf[:, :d] = rn(n, d).to(c.io)
    return NS(case=c, ids=ids, buf=buf, g=buf[:, :d], vocab=c.vocab)


# --------------------------------------------------------------- cross-entropy
CE_MUTANTS = ("no_max_subtraction", "mean_over_all_rows", "ignored_row_has_grad", "grad_ignores_gout",
              "row_stride_is_V", "sum_one_trip_only", "onehot_shifted")
EMB_MUTANTS = ("bf16_truncates", "pos_from_flat_index", "bad_row_not_zeroed", "lane_loop_one_trip")
TG_MUTANTS = ("tail_rows_dropped", "second_column_block_dropped", "oob_bin_written")
MUTANTS = CE_MUTANTS + EMB_MUTANTS + TG_MUTANTS


def ce_reference(x, targets, ignore_index=-100, gout=1.0):
    """float64; {"loss", "count", "lse", "dlogits"}."""
    xd = x.double()
    rows, V = xd.shape
    t = targets.reshape(-1).long()
    m = xd.max(1, keepdim=True).values
    lse = (m + (xd - m).exp().sum(1, keepdim=True).log())[:, 0]
    live = t != ignore_index
    ok = live & (t >= 0) & (t < V)
    picked = xd.gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
    zero = torch.zeros_like(lse)
    row = torch.where(live, torch.where(ok, lse - picked, torch.full_like(lse, NAN)), zero)
    count = live.sum().double()
    onehot = torch.zeros_like(xd)
    onehot[ok, t[ok]] = 1.0
    d = ((xd - lse[:, None]).exp() - onehot) * (gout / count)
    return {"loss": row.sum() / count, "count": count, "lse": lse,
            "dlogits": torch.where(live[:, None], d, torch.zeros_like(d))}


def _tree(t):
    """The 64-lane butterfly of wave_sum, as lane 0 sees it: pairwise over the last dimension."""
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _block_sums(v):
    """Per 256-thread block: 4 wave sums, then ((0 + w0) + w1) + w2) + w3."""
    nb = (v.numel() + CE_BLOCK - 1) // CE_BLOCK
    w = _tree(F.pad(v, (0, nb * CE_BLOCK - v.numel())).view(nb, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _ce_sum(part, one_trip=False):
    """ce_sum_kernel: thread i adds part[i], part[i + 256], ...; then one block sum."""
    trips = (part.numel() + CE_BLOCK - 1) // CE_BLOCK
    p = F.pad(part, (0, trips * CE_BLOCK - part.numel())).view(trips, CE_BLOCK)
    acc = torch.zeros(CE_BLOCK)
    for k in range(1 if one_trip else trips):
        acc = acc + p[k]
    return _block_sums(acc)[0]


def ce_restatement(x, targets, ignore_index=-100, gout=1.0, mutant=None):
    """csrc/loss.hip in float32 torch; the gradient in x's dtype."""
    assert mutant is None or mutant in CE_MUTANTS
    rows, V = x.shape
    if mutant == "row_stride_is_V":
        x = torch.as_strided(x, (rows, V), (V, 1))
    xf = x.float()
    t = targets.reshape(-1).long()
    m = torch.zeros(rows, 1) if mutant == "no_max_subtraction" else xf.max(1, keepdim=True).values
    e = (xf - m).exp()
    s = torch.zeros(rows)
    for v in range(V):
        s = s + e[:, v]
    lse = m[:, 0] + s.log()
    live = t != ignore_index
    ok = live & (t >= 0) & (t < V)
    picked = xf.gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
    zero = torch.zeros(rows)
    row = torch.where(live, torch.where(ok, lse - picked, torch.full((rows,), NAN)), zero)
    one_trip = mutant == "sum_one_trip_only"
    sa, sc = _ce_sum(_block_sums(row), one_trip), _ce_sum(_block_sums(live.float()), one_trip)
    if mutant == "mean_over_all_rows":
        sc = torch.tensor(float(rows))
    g = torch.tensor(1.0 if mutant == "grad_ignores_gout" else gout, dtype=F32)
    onehot = torch.zeros(rows, V)
    tt = (t + 1) % V if mutant == "onehot_shifted" else t
    onehot[ok, tt[ok]] = 1.0
    d = ((xf - lse[:, None]).exp() - onehot) * (g / sc)
    if mutant != "ignored_row_has_grad":
        d = torch.where(live[:, None], d, torch.zeros_like(d))
    return {"loss32": sa / sc, "loss": sa / sc, "count32": sc, "count": sc, "lse32": lse, "lse": lse,
            "dlogits32": d, "dlogits": d.to(x.dtype)}


# --------------------------------------------------------------- embedding sum
def bad_rows(i):
    c = i.case
    bad = (i.tok < 0) | (i.tok >= c.V)
    if c.layout == "at":
        bad = bad | (i.pid < 0) | (i.pid >= c.P)
    return bad


def embed_reference(i):
    """float64; {"y", "d_tok", "d_quant", "d_pos"} (the gradients where the case has them)."""
    c = i.case
    d = torch.float64
    bad = bad_rows(i)
    tok = i.tok.clamp(0, c.V - 1)
    pid = i.pid.long().clamp(0, c.P - 1)
    y = i.tw.to(d)[tok] + i.qw.to(d)[i.qid.long()] + i.pw.to(d)[pid]
    out = {"y": torch.where(bad[..., None], torch.zeros_like(y), y)}
    if c.grads:
        dy = i.dy.to(d)
        S = dy.sum(0)
        out["d_tok"] = torch.zeros(c.V, c.d, dtype=d).index_add_(0, i.tok.reshape(-1), dy.reshape(-1, c.d))
        out["d_quant"] = torch.zeros(c.Q, c.d, dtype=d).index_add_(0, i.qid.long(), S)
        out["d_pos"] = torch.zeros(c.P, c.d, dtype=d).index_add_(0, i.pid.long(), S)
    return out


def truncate_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (what round-to-nearest-even is not)."""
    return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def embed_restatement(i, mutant=None):
    """embed_sum_kernel and EmbedSumFn.backward in float32 torch."""
    assert mutant is None or mutant in EMB_MUTANTS
    c = i.case
    bad = bad_rows(i)
    tok = i.tok.clamp(0, c.V - 1)
    pid = i.pid.long().clamp(0, c.P - 1)
    if mutant == "pos_from_flat_index" and c.layout == "codec":
        pid = torch.arange(c.L)
    y = (i.tw[tok] + i.pw[pid]) + i.qw[i.qid.long()]
    if mutant != "bad_row_not_zeroed":
        y = torch.where(bad[..., None], torch.zeros_like(y), y)
    if mutant == "lane_loop_one_trip":
        y[..., 256:] = 0.0
    out = {"y32": y, "y": truncate_bf16(y) if mutant == "bf16_truncates" and c.io == BF16 else y.to(c.io)}
    if c.grads:
        dy = i.dy.float()
        S = dy.sum(0)
        g2d = i.dy.reshape(-1, c.d)
        if c.V <= EMB_BINS and c.d % 8 == 0:
            out["d_tok32"] = table_grad_restatement(i.tok.reshape(-1), g2d, c.V)["out32"]
        else:
            out["d_tok32"] = torch.zeros(c.V, c.d).index_add_(0, i.tok.reshape(-1), g2d.float())
        out["d_quant32"] = torch.zeros(c.Q, c.d).index_add_(0, i.qid.long(), S)
        out["d_pos32"] = torch.zeros(c.P, c.d).index_add_(0, i.pid.long(), S)
        for k in ("d_tok", "d_quant", "d_pos"):
            out[k] = out[k + "32"]
    return out


# ------------------------------------------------------------- table gradient
def table_grad_reference(ids, g, vocab):
    ok = (ids >= 0) & (ids < vocab)
    return {"out": torch.zeros(vocab, g.shape[1], dtype=torch.float64).index_add_(0, ids[ok], g[ok].double())}


def table_grad_restatement(ids, g, vocab, mutant=None, route="hip"):
    """embed_table_grad_kernel and its column sum in float32 torch; any other
    route of _table_grad: a float32 index_add_."""
    assert mutant is None or mutant in TG_MUTANTS
    n, d = g.shape
    if route != "hip":
        ok = (ids >= 0) & (ids < vocab)
        out = torch.zeros(vocab, d).index_add_(0, ids[ok], g[ok].float())
        return {"out32": out, "out": out}
    if mutant == "tail_rows_dropped":
        n -= n % 4
    rpb, nblk = emb_grad_blocks(n)
    idp = torch.full((nblk * rpb,), -1, dtype=torch.long)
    idp[:n] = ids[:n]
    if mutant == "oob_bin_written":
        live = (idp >= vocab) & (idp < EMB_BINS)
        idp = torch.where(live, idp % vocab, idp)
    gp = torch.zeros(nblk * rpb, d)
    gp[:n] = g[:n].float()
    idp, gp = idp.view(nblk, rpb // 4, 4), gp.view(nblk, rpb // 4, 4, d)
    bins = torch.arange(EMB_BINS).view(1, 1, EMB_BINS, 1)
    acc = torch.zeros(nblk, 4, EMB_BINS, d)
    for j in range(rpb // 4):         # wave w: rows r0 + w, r0 + w + 4, ...; fma(id == v, x, acc)
        acc = acc + (idp[:, j, :, None, None] == bins).float() * gp[:, j, :, None, :]
    part = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])            # (nblk, 16, d)
    # the column sum over the blocks: partial p goes to wave p % 4, running sum (p // 4) % 8
    trips = (nblk + 31) // 32
    p = F.pad(part, (0, 0, 0, 0, 0, trips * 32 - nblk)).view(trips, 8, 4, EMB_BINS, d)
    run = torch.zeros(8, 4, EMB_BINS, d)
    for k in range(trips):
        run = run + p[k]
    s = ((run[0] + run[1]) + (run[2] + run[3])) + ((run[4] + run[5]) + (run[6] + run[7]))
    out = ((s[0] + s[1]) + (s[2] + s[3]))[:vocab].clone()
    if mutant == "second_column_block_dropped":
        out[:, 64 * (16 // g.element_size()):] = 0.0
    return {"out32": out, "out": out}


def reference(i):
    if i.case.op == "ce":
        return ce_reference(i.x, i.t, i.ignore, i.gout)
    if i.case.op == "emb":
        return embed_reference(i)
    return table_grad_reference(i.ids, i.g, i.vocab)


def restatement(i, mutant=None):
    if i.case.op == "ce":
        return ce_restatement(i.x, i.t, i.ignore, i.gout, mutant)
    if i.case.op == "emb":
        return embed_restatement(i, mutant)
    return table_grad_restatement(i.ids, i.g, i.vocab, mutant, table_route(i.case))


def candidate(rest):
    """A restatement's outputs in the form a kernel run is handed to `check`."""
    return {k: v for k, v in rest.items() if not k.endswith("32")}


# ----------------------------------------------------------------- the criterion
def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def errors(got, ref, rest, dtype):
    """Per tensor of `got`: (excess, ratio, rel).  excess: the largest amount
    by which an element misses its bound, <= 0 when the tensor passes (inf for
    a wrong dtype or shape, a non-finite value out of place, a non-zero where
    the reference is exactly 0, a bit of difference in an EXACT tensor);
    ratio: max|got - ref| / max|rest32 - ref| over the finite elements, a bf16
    tensor less one rounding of its element; rel: that error / max|ref|."""
    res = {}
    fail = (math.inf, math.inf, math.inf)
    for k, g in got.items():
        g = g.detach().cpu()
        r, own, stored = ref[k].double(), rest[k + "32"].double(), rest[k]
        if g.dtype != stored.dtype or g.numel() != r.numel() or (k in IO_KEYS and g.dtype != dtype):
            res[k] = fail
            continue
        g = g.reshape(r.shape)
        gd = g.double()
        inf = torch.isinf(r)
        if not (torch.equal(torch.isnan(gd), torch.isnan(r)) and torch.equal(torch.isinf(gd), inf)
                and torch.equal(gd[inf], r[inf])):
            res[k] = fail
            continue
        if k in EXACT and not torch.equal(bits(g), bits(stored.reshape(r.shape))):
            res[k] = fail
            continue
        fin = torch.isfinite(r)
        gf, rf, of = gd[fin], r[fin], own[fin]
        if not rf.numel():
            res[k] = (0.0, 0.0, 0.0)
            continue
        if ((rf == 0) & (gf != 0)).any():
            res[k] = fail
            continue
        scale = rf.abs().max().item()
        own_err = (of - rf).abs().max().item()
        slack = RATIO * own_err + FLOOR * scale
        err = (gf - rf).abs()
        if g.dtype == BF16:
            err = (err - BF16_ULP * rf.abs()).clamp_min(0.0)
        else:
            assert g.dtype == F32, (k, g.dtype)
        worst = err.max().item()
        res[k] = (worst - slack, worst / own_err if own_err > 0 else (0.0 if worst == 0 else math.inf),
                  worst / scale if scale > 0 else worst)
    return res


def check(got, ref, rest, dtype, name=""):
    """Assert the criterion of the module docstring on every tensor of `got`;
    returns {tensor: (ratio, rel)} of `errors` for the record."""
    res = errors(got, ref, rest, dtype)
    bad = {k: v for k, v in res.items() if not v[0] <= 0}
    assert not bad, f"{name}: " + ", ".join(f"{k}: over its bound by {e:.3e} (ratio {q:.2f})"
                                            for k, (e, q, _) in bad.items())
    return {k: v[1:] for k, v in res.items()}
