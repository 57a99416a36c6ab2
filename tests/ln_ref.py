"""The comparison that pins LayerNorm (+ residual, + FiLM) forward and backward
(csrc/ln.hip through mtts.ops.layer_norm), shared by tests/test_ln_ref_cpu.py
(which proves it on the CPU: the closed form against float64 autograd, the
criterion against the listed mutants) and tests/test_gpu_layernorm.py (which
checks the kernels against it).

`reference`: float64, closed form.
    S = x + res; mean, var (biased) over a row; rstd = 1 / sqrt(var + eps)
    xhat = (S - mean) rstd; ln = xhat w + b; y = gamma_g ln + beta_g
    dxhat = dy gamma_g w
    dS = dsum + rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat))
    dw = sum dy gamma_g xhat, db = sum dy gamma_g        (all rows)
    dgamma_g = sum dy ln, dbeta_g = sum dy               (the rows of group g)
For bf16 I/O the kernel rounds S to bf16 before its statistics, so that both
passes see the stored stream value; the reference does the same (x + res in
fp32, then bf16) and treats that S as the leaf.  Its `x_sum` stays the exact
x + res: the stored value must lie within one rounding of it.

`restatement`: the same formulas in float32 torch, in the kernel's form (two
running sums A = sum dy xhat, S = sum dy per FiLM group: dw = sum_g gamma_g A_g,
dgamma = w A + b S), outputs rounded to the I/O dtype; the values before that
rounding are kept under "<name>32".  Its own distance to the reference is the
yardstick of `check`, measured per case, since it grows with the inputs (1e-7
to 3e-7 of a tensor's maximum for unit-normal inputs, 3e-6 when they are offset
by +100).

`check(got, ref, rest, io_dtype)`: per tensor, scale = max|ref|,
    slack = 8 max|rest32 - ref| + 1e-6 scale
    a float32 tensor:  max|got - ref| <= slack
    a bfloat16 tensor: |got - ref| <= 2^-8 |ref| + slack     elementwise
The kernel and the restatement are both fp32 with the same roundings per
element and differ in summation order (a 64-lane tree and per-block partials
against torch's order); 8x leaves room for that and nothing else.  The nearest
mutant (eps outside the square root, rows of variance 2e-4) sits at 2.4e-2.  A
tensor is judged by its own dtype: y, dx, dres and x_sum follow the I/O dtype,
dgamma and dbeta follow gamma's (autograd hands a bf16 gamma a bf16 gradient).

The slot's column sums (`dx_colsum`) are defined by the dx stored beside them:
they are compared with the float64 column sums of got["dx"], the yardstick
being torch's fp32 sum of the same rows.  Sums of the reference's own dS would
fold every one-ulp difference in a bf16 dx (2^-9 of an element) into a sum
whose fp32 error is 1e-7.

CASES is the list both files run.  A case fixes the shapes, dtypes, FiLM
grouping, eps and the kind of inputs; layouts and the three ways of passing
FiLM are the GPU file's business (they do not change the values)."""
import functools
import math
import types
import zlib

import torch

F32, BF16 = torch.float32, torch.bfloat16
RATIO = 8.0        # kernel error / restatement error allowed
FLOOR = 1e-6       # of the tensor's maximum
BF16_ULP = 2.0 ** -8


# ------------------------------------------------------------------- the cases
def Case(name, rows, cols, io, gb=None, G=0, rpg=0, res=True, eps=1e-5, kind="normal", dy=True, dsum=True,
         lead=None):
    """rows x cols in `io`; gb: gamma / beta dtype (None: no FiLM), G groups of
    rpg rows; kind: "normal", "small" (x, res * 1e-2), "offset" (x + 100),
    "const_row" (row 3 constant), "row_scales" (odd rows * 1e3); dy / dsum:
    whether y / x_sum receive a gradient; lead: leading shape of x when not (rows,)."""
    assert gb is None or G * rpg == rows
    return types.SimpleNamespace(name=name, rows=rows, cols=cols, io=io, gb=gb, G=G, rpg=rpg, res=res, eps=eps,
                                 kind=kind, dy=dy, dsum=dsum and res, lead=lead or (rows,))


def _tag(dt):
    return {F32: "f32", BF16: "bf16", None: "none"}[dt]


def _cases():
    out = []
    # 1. every instantiation dispatch_ln can take (rows = 37: rb = 8, last block ragged)
    vec = {F32: (256, 512, 768, 1024, 1536, 2048), BF16: (512, 1024, 1536, 2048, 3072, 4096)}
    scalar = {F32: (64, 128, 192, 384), BF16: (64, 128, 192, 384, 256)}
    for io in (F32, BF16):
        out += [Case(f"vec-{_tag(io)}-{c}", 37, c, io) for c in vec[io]]
        out += [Case(f"scalar-{_tag(io)}-{c}", 37, c, io) for c in scalar[io]]
        out += [Case(f"forced-{_tag(io)}-{c}", 37, c, io) for c in (256, 512, 1024)]
    # 2. row blocks of the backward without FiLM, and the 4-wave backward's ragged block
    for io in (F32, BF16):
        out += [Case(f"rows-{_tag(io)}-{r}", r, 64, io) for r in (1, 3, 8, 9, 2049, 4097, 8193, 16385)]
    out += [Case("wave4-f32-2048", 9, 2048, F32), Case("wave4-bf16-4096", 9, 4096, BF16)]
    # 3. FiLM groups: every T / TG pair
    for cols in (128, 1024):
        for G, rpg in ((3, 1), (7, 2), (5, 17), (4, 96), (3, 64), (2, 192), (1, 40)):
            for io in (F32, BF16):
                for gb in (F32, BF16):
                    out.append(Case(f"film-{cols}-{G}x{rpg}-{_tag(io)}-{_tag(gb)}", G * rpg, cols, io, gb, G, rpg))
    # 4. strides: (2, 19, 512), one FiLM group per batch row (rb = 1)
    out += [Case(f"strides-{_tag(io)}", 38, 512, io, F32, 2, 19, lead=(2, 19)) for io in (F32, BF16)]
    # 5. options
    for io in (F32, BF16):
        t = _tag(io)
        out += [Case(f"opt-nores-{t}", 37, 256, io, res=False),
                Case(f"opt-nores-film-{t}", 40, 512, io, F32, 2, 20, res=False),
                Case(f"opt-yonly-{t}", 37, 512, io, dsum=False),
                Case(f"opt-sumonly-{t}", 37, 512, io, dy=False),
                Case(f"opt-film-yonly-{t}", 40, 512, io, F32, 2, 20, dsum=False),
                Case(f"opt-film-{t}", 40, 512, io, F32, 2, 20)]
    # 6. numerics
    for kind in ("small", "offset", "const_row", "row_scales"):
        for eps in (1e-5, 1e-6):
            for io in (F32, BF16):
                out.append(Case(f"num-{kind}-{eps:g}-{_tag(io)}", 40, 1024, io, F32, 2, 20, eps=eps, kind=kind))
    # 8. determinism: 3001 blocks of one row, one group
    out.append(Case("determinism-bf16", 3001, 256, BF16, F32, 1, 3001))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def row_block(rows, rpg=None):
    """ln_rb of csrc/ln.hip: the backward's rows per block."""
    if not rpg:
        rb = 64
        while rb > 8 and (rows + rb - 1) // rb < 256:
            rb >>= 1
        return rb
    rb = 64
    while rb > 1 and rpg % rb:
        rb >>= 1
    return rb


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """CPU tensors of a case, (rows, cols) and (G, cols), in the dtypes the kernel is given."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    x, res = rn(c.rows, c.cols), rn(c.rows, c.cols)
    if c.kind == "small":
        x, res = x * 1e-2, res * 1e-2
    elif c.kind == "offset":
        x = x + 100.0
    elif c.kind == "const_row":
        x[3], res[3] = 0.5, 0.25 if c.res else 0.0
    elif c.kind == "row_scales":
        x[1::2] *= 1e3
        res[1::2] *= 1e3
    i = types.SimpleNamespace(case=c, eps=c.eps, x=x.to(c.io), res=res.to(c.io) if c.res else None,
                              w=1 + 0.1 * rn(c.cols), b=0.1 * rn(c.cols), gamma=None, beta=None,
                              dy=rn(c.rows, c.cols).to(c.io) if c.dy else None,
                              dsum=rn(c.rows, c.cols).to(c.io) if c.dsum else None)
    if c.gb is not None:
        i.gamma, i.beta = rn(c.G, c.cols).to(c.gb), rn(c.G, c.cols).to(c.gb)
    return i


# ---------------------------------------------------------- float64 closed form
def stream(i, dtype=torch.float64):
    """(the exact x + res, the S the statistics see) in `dtype`."""
    c = i.case
    if i.res is None:
        return None, i.x.to(dtype)
    exact = i.x.double() + i.res.double()
    if c.io == BF16:       # fp32 add (exact sum, one rounding), then the stored bf16 value
        return exact.to(dtype), exact.float().bfloat16().to(dtype)
    return exact.to(dtype), exact.to(dtype)


def reference(i):
    """The float64 closed form of the module docstring; a dict of float64 tensors."""
    c = i.case
    d = torch.float64
    exact, S = stream(i)
    w, b = i.w.to(d), i.b.to(d)
    mean = S.mean(-1, keepdim=True)
    var = ((S - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + c.eps)
    xhat = (S - mean) * rstd
    ln = xhat * w + b
    film = i.gamma is not None
    grp = torch.arange(c.rows) // c.rpg if film else None
    gam = i.gamma.to(d)[grp] if film else torch.ones((), dtype=d)
    y = gam * ln + i.beta.to(d)[grp] if film else ln
    dy = i.dy.to(d) if i.dy is not None else torch.zeros_like(S)
    dxhat = dy * gam * w
    dS = rstd * (dxhat - dxhat.mean(-1, keepdim=True) - xhat * (dxhat * xhat).mean(-1, keepdim=True))
    if i.dsum is not None:
        dS = dS + i.dsum.to(d)
    out = {"y": y, "dx": dS, "dw": (dy * gam * xhat).sum(0), "db": (dy * gam).expand_as(dy).sum(0),
           "mean": mean[:, 0], "rstd": rstd[:, 0]}
    if exact is not None:
        out["x_sum"], out["dres"] = exact, dS
    if film:
        out["dgamma"] = (dy * ln).view(c.G, c.rpg, c.cols).sum(1)
        out["dbeta"] = dy.view(c.G, c.rpg, c.cols).sum(1)
    return out


# ------------------------------------------------------ the kernel in fp32 torch
MUTANTS = ("var_n_minus_1", "eps_outside_sqrt", "eps_dropped", "dx_no_xhat_term", "dgamma_no_bias_term",
           "film_group_per_64_rows", "ragged_block_dropped", "colsum_before_rounding")


def restatement(i, mutant=None):
    """csrc/ln.hip in float32 torch on the CPU.  "<name>": the output as the
    kernel stores it; "<name>32": before the rounding to the storage dtype.
    dx_colsum: the fp32 column sums of dx as stored."""
    assert mutant is None or mutant in MUTANTS
    c = i.case
    n = c.cols
    _, S = stream(i, F32)
    out = {}
    if i.res is not None:
        out["x_sum32"] = i.x.float() + i.res.float()
    w, b = i.w.float(), i.b.float()
    eps = torch.tensor(c.eps, dtype=F32)
    mean = S.sum(-1, keepdim=True) / n
    dev = S - mean
    var = (dev * dev).sum(-1, keepdim=True) / (n - 1 if mutant == "var_n_minus_1" else n)
    if mutant == "eps_outside_sqrt":
        rstd = 1.0 / (torch.sqrt(var) + eps)
    elif mutant == "eps_dropped":
        rstd = 1.0 / torch.sqrt(var)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    xhat = dev * rstd
    ln = xhat * w + b
    film = i.gamma is not None
    G = c.G if film else 1
    r = torch.arange(c.rows)
    if film:
        grp = (r // 64 * 64 if mutant == "film_group_per_64_rows" and c.rpg % 64 else r) // c.rpg
        gamma, beta = i.gamma.float(), i.beta.float()
    else:
        grp = torch.zeros(c.rows, dtype=torch.long)
        gamma = torch.ones(1, n)
    gam = gamma[grp]
    out["y32"] = gam * ln + beta[grp] if film else ln
    dy = i.dy.float() if i.dy is not None else torch.zeros_like(S)
    dxhat = dy * gam * w
    m1 = dxhat.sum(-1, keepdim=True) / n
    m2 = (dxhat * xhat).sum(-1, keepdim=True) / n
    dx = rstd * (dxhat - m1 - (0 if mutant == "dx_no_xhat_term" else xhat * m2))
    if i.dsum is not None:
        dx = dx + i.dsum.float()
    out["dx32"] = dx
    keep = c.rows
    if mutant == "ragged_block_dropped" and not film:
        keep = c.rows // row_block(c.rows) * row_block(c.rows)
    if film and mutant == "film_group_per_64_rows":
        A = torch.zeros(G, n).index_add_(0, grp, dy * xhat)
        Sm = torch.zeros(G, n).index_add_(0, grp, dy)
    else:       # torch's blocked sum over a group's rows, as the kernel's is (per wave, per block, per group)
        A = (dy * xhat)[:keep].view(G, keep // G, n).sum(1)
        Sm = dy[:keep].view(G, keep // G, n).sum(1)
    out["dw32"], out["db32"] = (gamma * A).sum(0), (gamma * Sm).sum(0)
    if film:
        out["dgamma32"] = w * A if mutant == "dgamma_no_bias_term" else w * A + b * Sm
        out["dbeta32"] = Sm
    out["mean32"], out["rstd32"] = mean[:, 0], rstd[:, 0]
    stored = {"y": c.io, "dx": c.io, "x_sum": c.io, "dgamma": c.gb, "dbeta": c.gb}
    for k in [k[:-2] for k in out]:
        out[k] = out[k + "32"].to(stored.get(k, F32))
    if i.res is not None:
        out["dres"], out["dres32"] = out["dx"], out["dx32"]
    out["dx_colsum"] = (out["dx32"] if mutant == "colsum_before_rounding" else out["dx"].float()).sum(0)
    return out


OUTPUTS = ("y", "x_sum", "dx", "dres", "dw", "db", "dgamma", "dbeta", "dx_colsum", "mean", "rstd")


def candidate(rest):
    """A restatement's outputs in the form a kernel run is handed to `check`."""
    return {k: rest[k] for k in OUTPUTS if k in rest}


# ----------------------------------------------------------------- the criterion
def errors(got, ref, rest, io_dtype):
    """Per tensor of `got`: (excess, ratio, rel).  excess: the largest amount
    by which an element misses its bound, <= 0 when the tensor passes; err:
    max|got - ref|, less one bf16 rounding where the tensor is bf16; ratio:
    err / max|rest32 - ref|, the figure the GPU file records (inf where the
    restatement is exact and the kernel is not: few-term sums of bf16 values,
    which the floor then decides); rel: err / max|ref|."""
    res = {}
    for k, g in got.items():
        assert k in OUTPUTS, k
        g = g.detach().cpu()
        if k == "dx_colsum":
            stored = got["dx"].detach().cpu().reshape(-1, g.shape[-1])
            r, own = stored.double().sum(0), stored.float().sum(0).double()
        else:
            r, own = ref[k], rest[k + "32"].double()
        if k in ("y", "x_sum", "dx", "dres"):
            assert g.dtype == io_dtype, (k, g.dtype)
        g = g.reshape(r.shape)
        if not torch.isfinite(g).all():
            res[k] = (math.inf, math.inf, math.inf)
            continue
        scale = r.abs().max().item() if r.numel() else 0.0
        own_err = (own - r).abs().max().item() if r.numel() else 0.0
        slack = RATIO * own_err + FLOOR * scale
        err = (g.double() - r).abs()
        if g.dtype == BF16:
            err = (err - BF16_ULP * r.abs()).clamp_min(0.0)
        else:
            assert g.dtype == F32, (k, g.dtype)
        worst = err.max().item() if r.numel() else 0.0
        res[k] = (worst - slack, worst / own_err if own_err > 0 else (0.0 if worst == 0 else math.inf),
                  worst / scale if scale > 0 else worst)
    return res


def check(got, ref, rest, io_dtype, name=""):
    """Assert the criterion of the module docstring on every tensor of `got`;
    returns {tensor: (ratio, rel)} of `errors` for the record."""
    res = errors(got, ref, rest, io_dtype)
    bad = {k: v for k, v in res.items() if not v[0] <= 0}
    assert not bad, f"{name}: " + ", ".join(f"{k}: over its bound by {e:.3e} (ratio {q:.2f})"
                                            for k, (e, q, _) in bad.items())
    return {k: v[1:] for k, v in res.items()}
