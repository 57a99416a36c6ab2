"""LayerNorm (+ residual, + FiLM) forward and backward (csrc/ln.hip) through
mtts.ops.layer_norm, as the decoder calls it, against the float64 closed form
of tests/ln_ref.py under its criterion (ln_ref.check; proven on the CPU by
tests/test_ln_ref_cpu.py): every instantiation dispatch_ln can take, every
row-block size of the backward, FiLM groups of 1, 2, odd, 64-divisible and
64-indivisible row counts in all four dtype pairs and three ways of passing
them, strided and misaligned inputs and gradients, the optional outputs,
inputs on which eps and cancellation matter, the host-side validation, and
run-to-run determinism.

Besides the criterion, x_sum is compared bit for bit: it is one fp32 add,
rounded once to the storage dtype.

Measured on an MI355X, the largest kernel-to-restatement ratio per tensor over
all cases (max|kernel - reference| / max|restatement - reference|, a bf16
tensor less one rounding of its element; the bound is 8), the case it occurs
at and the kernel's error there as a fraction of the tensor's maximum:

    y          1.32  1.6e-07  film-1024-3x64-f32-bf16
    x_sum      1.00  3.9e-08  vec-f32-256  (and bit-identical everywhere)
    dx, dres   1.61  9.1e-08  rows-f32-3
    dw         1.67  2.1e-07  film-128-7x2-f32-bf16
    db         3.34  9.8e-08  film-1024-1x40-bf16-f32
    dgamma     1.75  1.9e-07  film-1024-7x2-f32-f32
    dbeta      1.33  1.0e-07  film-128-4x96-f32-f32
    mean       1.25  1.4e-07  scalar-f32-384
    rstd       1.90  9.4e-08  scalar-bf16-128
    dx_colsum  15.0  2.3e-08  scalar-bf16-128

dx_colsum is the one above 8, and by the arithmetic, not the kernel: a sum of
37 bf16 values is exact in fp32 but for its smallest terms, so torch's fp32 sum
of the stored dx, the yardstick, is off by 1.5e-9 of the maximum there and the
kernel's per-wave, per-block order by 2.3e-8; the criterion's 1e-6 floor
decides, as it does where the restatement is exact (db up to 6.7e-9, mean up to
2.3e-8 of the maximum on bf16 cases).  Set MTTS_LN_RATIOS=<file> to have a run
write this table."""
import ctypes as C
import functools
import math
import os

import pytest
import torch

import ln_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")

# tensor -> [largest finite ratio, its case, err / max|ref| there, err / max|ref| where the restatement is exact]
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    path = os.environ.get("MTTS_LN_RATIOS")
    if path and _RATIOS:
        with open(path, "w") as fh:
            fh.write(f"{'tensor':<10} {'ratio':>7}  {'err/max':>8}  {'case':<28} err/max, restatement exact\n")
            for k in R.OUTPUTS:
                if k in _RATIOS:
                    q, name, rel, rel0 = _RATIOS[k]
                    fh.write(f"{k:<10} {q:7.2f}  {rel:8.1e}  {name:<28} {rel0:.1e}\n")


def place(t, lead, layout):
    """The (rows, cols) CPU tensor on the device as (*lead, cols): "contig";
    "aligned": inside a wider and longer NaN-filled buffer, rows and pointer
    on 16-byte boundaries; "element": at element offset 1 into rows of stride
    cols + 3, NaN around it."""
    if t is None:
        return None
    rows, cols = t.shape
    if layout == "contig":
        return t.to(DEV).unflatten(0, lead)
    if layout == "aligned":
        buf = torch.full((rows + 2, cols + 32), NAN, dtype=t.dtype, device=DEV)
        v = buf[1:rows + 1, 16:16 + cols]
        assert v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
    else:
        assert layout == "element"
        buf = torch.full((rows + 1, cols + 3), NAN, dtype=t.dtype, device=DEV)
        v = buf[:rows, 1:1 + cols]
        assert v.data_ptr() % 16 != 0 and (v.stride(0) * v.element_size()) % 16 != 0
    v.copy_(t)
    return v.unflatten(0, lead)


def run(name, form="split", layout="contig", grad_layout="contig", slot=False, stats=False):
    """One forward and backward of a case through ops.layer_norm; the outputs
    and gradients on the CPU, named as ln_ref names them."""
    from mtts import ops
    from mtts.linear import BiasGradSlot
    i = R.make_inputs(name)
    c = i.case
    n = c.cols
    x = place(i.x, c.lead, layout).requires_grad_(True)
    res = place(i.res, c.lead, layout)
    if res is not None:
        res.requires_grad_(True)
    w, b = i.w.to(DEV).requires_grad_(True), i.b.to(DEV).requires_grad_(True)
    kw, parent = {}, None
    if c.gb is not None:
        if form == "split":
            gam, bet = i.gamma.to(DEV).requires_grad_(True), i.beta.to(DEV).requires_grad_(True)
            kw = dict(gamma=gam, beta=bet)
        else:
            film = torch.cat([i.gamma, i.beta], 1).to(DEV)
            if form == "slice":      # one layer's share of a batched style MLP
                parent = torch.randn(c.G, 3 * 2 * n, device=DEV).to(c.gb)
                parent[:, 2 * n:4 * n] = film
                parent.requires_grad_(True)
                film = parent[:, 2 * n:4 * n]
            else:
                assert form == "tensor"
                film.requires_grad_(True)
            kw = dict(film=film)
        kw["rows_per_group"] = c.rpg
    s = BiasGradSlot() if slot else None
    y, xs = ops.layer_norm(x, w, b, c.eps, res=res, colsum_slot=s, **kw)
    assert y.shape == x.shape and y.dtype == c.io
    got = {"y": y}
    if res is not None:
        assert xs.shape == x.shape and xs.dtype == c.io
        got["x_sum"] = xs
    else:
        assert xs.numel() == 0 and not xs.requires_grad
    outs = [t for t, g in ((y, i.dy), (xs, i.dsum)) if g is not None]
    grads = [place(g, c.lead, grad_layout) for g in (i.dy, i.dsum) if g is not None]
    torch.autograd.backward(outs, grads)
    got.update(dx=x.grad, dw=w.grad, db=b.grad)
    if res is not None:
        got["dres"] = res.grad
    if c.gb is not None:
        if form == "split":
            got.update(dgamma=gam.grad, dbeta=bet.grad)
        else:
            g = film.grad if parent is None else parent.grad[:, 2 * n:4 * n]
            assert g.shape == (c.G, 2 * n)
            got.update(dgamma=g[:, :n], dbeta=g[:, n:])
            if parent is not None:       # the gradient arrives in the parent, zeros elsewhere
                assert parent.grad.shape == parent.shape
                assert not parent.grad[:, :2 * n].any() and not parent.grad[:, 4 * n:].any()
    if slot:
        cs = s.take(n)
        assert cs is not None and cs.dtype == F32 and cs.shape == (n,)
        got["dx_colsum"] = cs
    if stats:      # the saved statistics, which layer_norm keeps to itself
        assert c.gb is None
        with torch.no_grad():
            y2, mean, rstd, _ = ops.layernorm_fwd(x.detach(), w.detach(), b.detach(), c.eps,
                                                  res=None if res is None else res.detach())
        assert torch.equal(y2, y)
        got.update(mean=mean, rstd=rstd)
    return {k: v.detach().cpu() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(reference, restatement) of a case, computed once and only read."""
    i = R.make_inputs(name)
    return R.reference(i), R.restatement(i)


def compare(name, got):
    i = R.make_inputs(name)
    c = i.case
    ratios = R.check(got, *expected(name), c.io, name)
    for k, (q, rel) in ratios.items():
        row = _RATIOS.setdefault(k, [0.0, "-", 0.0, 0.0])
        if q == math.inf:
            row[3] = max(row[3], rel)
        elif q > row[0]:
            row[:3] = q, name, rel
    want = {"y", "dx", "dw", "db"} | ({"x_sum", "dres"} if c.res else set()) | \
        ({"dgamma", "dbeta"} if c.gb is not None else set())
    assert want <= set(ratios), sorted(want - set(ratios))
    if c.res:      # one fp32 add, one rounding
        assert torch.equal(got["x_sum"].reshape(c.rows, c.cols), R.stream(i, c.io)[1]), f"{name}: x_sum"
        assert torch.equal(got["dres"], got["dx"])
    return ratios


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def names(prefix):
    return [c.name for c in R.CASES if c.name.startswith(prefix)]


# ------------------------------------------------------------ 1. the dispatch
@pytest.mark.parametrize("name", names("vec-") + names("scalar-"))
def test_every_column_case(name):
    compare(name, run(name, slot=True, stats=True))


@pytest.mark.parametrize("name", names("forced-"))
def test_element_path_forced_by_misalignment(name):
    """NV = 4, 8, 16 of the element path: x, res and both gradients at element
    offset 1 into rows of stride cols + 3."""
    compare(name, run(name, layout="element", grad_layout="element", slot=True, stats=True))


@pytest.mark.parametrize("io,cols", [(io, c) for io in (F32, BF16) for c in (100, 320, 448, 640)]
                         + [(F32, 1280), (F32, 4096)])
def test_unsupported_cols_are_rejected(io, cols):
    from mtts import ops
    x = torch.randn(37, cols, device=DEV).to(io)
    w, b = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
    with pytest.raises(RuntimeError, match=f"cols={cols} "):
        ops.layer_norm(x, w, b, 1e-5, res=x.clone())
    with pytest.raises(RuntimeError, match=f"cols={cols} "):
        ops.layernorm_bwd(x, w, b, 1e-5, None, None, 1, torch.zeros(37, device=DEV), torch.ones(37, device=DEV), x)


# ---------------------------------------------------------- 2. the row blocks
@pytest.mark.parametrize("name", names("rows-") + names("wave4-"))
def test_row_blocks(name):
    """rb = 8, 16, 32, 64 with a last block of one row; fewer rows than a
    block has waves; the 4-wave backward's ragged block."""
    compare(name, run(name, slot=True))


# ---------------------------------------------------------- 3. the FiLM groups
@pytest.mark.parametrize("name", names("film-"))
def test_film_groups(name):
    split = run(name, form="split")
    compare(name, split)
    tensor = run(name, form="tensor", slot=True)
    compare(name, tensor)
    sliced = run(name, form="slice", slot=True)
    compare(name, sliced)
    same(tensor, sliced, "film tensor against its column slice")
    tensor.pop("dx_colsum")
    same(split, tensor, "gamma / beta against one film tensor")


# -------------------------------------------------------------- 4. the strides
@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_strided_inputs_and_gradients(io):
    name = f"strides-{io}"
    base = run(name, form="tensor", slot=True)
    compare(name, base)
    assert base["y"].shape == (2, 19, 512) and base["dx"].shape == (2, 19, 512)
    for layout in ("aligned", "element"):
        for lay_in, lay_grad in ((layout, "contig"), ("contig", layout), (layout, layout)):
            got = run(name, form="tensor", layout=lay_in, grad_layout=lay_grad, slot=True)
            compare(name, got)       # finite, too: the padding is NaN
            if layout == "aligned":
                same(base, got, f"x {lay_in}, gradients {lay_grad}")


def test_uncollapsible_leading_dims_raise():
    from mtts import ops
    x = torch.randn(2, 40, 512, device=DEV)[:, :19]
    w, b = torch.ones(512, device=DEV), torch.zeros(512, device=DEV)
    with pytest.raises(ValueError, match="collapsible"):
        ops.layer_norm(x, w, b)
    with pytest.raises(ValueError, match="collapsible"):
        ops.layer_norm(x.contiguous(), w, b, res=x)


def test_expanded_gradient_is_taken():
    """sum over the batch hands the backward a gradient with a zero batch
    stride, which is no (rows, stride) view: it is copied, not refused."""
    from mtts import ops
    i = R.make_inputs("strides-f32")
    x = i.x.to(DEV).view(2, 19, 512).requires_grad_(True)
    w, b = i.w.to(DEV), i.b.to(DEV)
    g = torch.randn(19, 512, device=DEV)
    y, _ = ops.layer_norm(x, w, b)
    (y.sum(0) * g).sum().backward()
    x2 = x.detach().clone().requires_grad_(True)
    y2, _ = ops.layer_norm(x2, w, b)
    y2.backward(g.expand(2, 19, 512).contiguous())
    assert torch.equal(x.grad, x2.grad)


# -------------------------------------------------------------- 5. the options
@pytest.mark.parametrize("name", names("opt-"))
@pytest.mark.parametrize("slot", [False, True], ids=["noslot", "slot"])
def test_options(name, slot, monkeypatch):
    """No residual (x_sum empty, not differentiable: asserted in run); only y
    or only x_sum used; the slot with and without FiLM, with and without a
    gradient of x_sum."""
    from mtts import ops
    seen = []
    inner = ops.layernorm_bwd

    def spy(*a, **k):
        seen.append(k.get("dx_acc"))
        return inner(*a, **k)
    monkeypatch.setattr(ops, "layernorm_bwd", spy)
    c = R.BY_NAME[name]
    got = run(name, form="tensor", slot=slot)
    compare(name, got)
    assert len(seen) == 1 and (seen[0] is None) == (not c.dsum)      # no dx_acc pass without an x_sum gradient
    if not c.dy:       # dy absent: dx is the x_sum gradient itself
        assert torch.equal(got["dx"], R.make_inputs(name).dsum)
        assert not got["dw"].any() and not got["db"].any()


@pytest.mark.parametrize("io", [F32, BF16])
@pytest.mark.parametrize("film", [False, True])
def test_zero_rows(io, film):
    from mtts import ops
    from mtts.linear import BiasGradSlot
    n = 256
    x = torch.empty(0, n, device=DEV, dtype=io, requires_grad=True)
    res = torch.empty(0, n, device=DEV, dtype=io, requires_grad=True)
    w, b = torch.ones(n, device=DEV, requires_grad=True), torch.zeros(n, device=DEV, requires_grad=True)
    fl = torch.empty(0, 2 * n, device=DEV, requires_grad=True) if film else None
    slot = BiasGradSlot()
    y, xs = ops.layer_norm(x, w, b, 1e-5, res=res, film=fl, rows_per_group=5, colsum_slot=slot)
    assert y.shape == (0, n) and xs.shape == (0, n)
    (y.float().sum() + xs.float().sum()).backward()
    assert x.grad.shape == (0, n) and res.grad.shape == (0, n)
    assert w.grad.shape == (n,) and not w.grad.any() and not b.grad.any()
    assert not slot.take(n).any()
    if film:
        assert fl.grad.shape == (0, 2 * n)


# ------------------------------------------------------------- 6. the numerics
@pytest.mark.parametrize("name", names("num-"))
def test_numerics(name):
    """Rows of variance 2e-4 (eps matters), inputs offset by +100, a constant
    row, rows 1e3 apart, at eps 1e-5 and 1e-6."""
    got = run(name, form="tensor", slot=True)
    compare(name, got)
    i = R.make_inputs(name)
    c = i.case
    if c.kind == "const_row":      # variance 0: xhat = 0, y = gamma b + beta in one fma
        g = 3 // c.rpg
        want = (i.gamma[g].double() * i.b.double() + i.beta[g].double()).float().to(c.io)
        assert torch.equal(got["y"][3], want)
        assert torch.isfinite(got["dx"][3]).all()


# ----------------------------------------------------------- 7. the validation
def test_group_count_and_film_width_are_validated():
    from mtts import ops
    n = 256
    x = torch.randn(10, n, device=DEV)
    w, b = torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    gb = lambda g, width=n: torch.randn(g, width, device=DEV)
    with pytest.raises(ValueError, match="rows_per_group=4"):
        ops.layer_norm(x, w, b, gamma=gb(3), beta=gb(3), rows_per_group=4)        # 10 % 4 != 0
    with pytest.raises(ValueError, match="3 FiLM groups"):
        ops.layer_norm(x, w, b, gamma=gb(3), beta=gb(3), rows_per_group=5)        # 2 groups, not 3
    with pytest.raises(ValueError, match="1 FiLM groups"):
        ops.layer_norm(x, w, b, film=gb(1, 2 * n), rows_per_group=5)
    with pytest.raises(ValueError, match="beta"):
        ops.layer_norm(x, w, b, gamma=gb(2), beta=gb(1), rows_per_group=5)
    with pytest.raises(ValueError, match="film must be"):
        ops.layer_norm(x, w, b, film=gb(2, n), rows_per_group=5)
    with pytest.raises(ValueError, match="film must be"):
        ops.layer_norm(x, w, b, film=gb(2, 2 * n + 8), rows_per_group=5)
    y, _ = ops.layer_norm(x, w, b, film=gb(2, 2 * n), rows_per_group=5)
    assert torch.isfinite(y).all()


def test_c_entry_points_reject_a_ragged_last_group():
    """rows % rows_per_group != 0 straight at the C ABI: an error that names
    both numbers, from the forward and from the backward."""
    from mtts import _lib as L
    from mtts import ops
    n, rows, rpg = 256, 10, 4
    z = lambda *s: torch.zeros(*s, device=DEV)
    x, y, w, b, mean, rstd = z(rows, n), z(rows, n), z(n), z(n), z(rows), z(rows)
    gam, bet = z(3, n), z(3, n)          # ceil(10 / 4) rows: nothing lies outside them either way
    a = ops._ln_args(x, w, b, 1e-5, None, None, gam, bet, rpg, y, mean, rstd)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.lib()
    assert lib.mtts_layernorm_fwd(C.byref(a), stream) != 0
    msg = lib.mtts_last_error().decode()
    assert "rows=10" in msg and "rows_per_group=4" in msg, msg
    with pytest.raises(RuntimeError, match="rows=10 .*rows_per_group=4"):
        L.call("mtts_layernorm_fwd", a)
    bb = L.LNBwdArgs()
    bb.f = a
    dy, dx, dw, db, dg, dbe = z(rows, n), z(rows, n), z(n), z(n), z(3, n), z(3, n)
    ws = torch.empty(lib.mtts_layernorm_bwd_workspace(rows, n, rpg), device=DEV, dtype=torch.uint8)
    bb.dy, bb.dy_rs, bb.dx, bb.dx_rs = dy.data_ptr(), n, dx.data_ptr(), n
    bb.dw, bb.db, bb.dgamma, bb.dbeta, bb.workspace = (t.data_ptr() for t in (dw, db, dg, dbe, ws))
    assert lib.mtts_layernorm_bwd(C.byref(bb), stream) != 0
    msg = lib.mtts_last_error().decode()
    assert "rows=10" in msg and "rows_per_group=4" in msg, msg
    torch.cuda.synchronize()
    assert not y.any() and not dx.any()       # nothing was launched


# ---------------------------------------------------------- 8. the determinism
def test_two_runs_are_bit_identical():
    name = "determinism-bf16"
    a = run(name, form="tensor", slot=True)
    b = run(name, form="tensor", slot=True)
    same(a, b, "second run")
    compare(name, a)
