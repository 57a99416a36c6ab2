"""tests/ln_ref.py proven on the CPU: the float64 closed form against float64
autograd through torch's own layer_norm, the float32 restatement of
csrc/ln.hip against the criterion on every case the GPU file runs, and the
criterion against the mutants it has to tell from a right kernel.

Measured here (max|restatement - reference| / max|reference|, over CASES):
unit-normal inputs 6e-8 to 4e-7 per tensor, +100 offset up to 4e-6 (y, dx).
The nearest mutant is `eps_outside_sqrt` on the variance-2e-4 rows of
num-small-*: 2.4e-2 at eps = 1e-5, 2.5e-3 at eps = 1e-6."""
import pytest
import torch
import torch.nn.functional as F

import ln_ref as R

NAMES = [c.name for c in R.CASES]


def _run(name, mutant=None):
    i = R.make_inputs(name)
    ref, rest = R.reference(i), R.restatement(i)
    cand = rest if mutant is None else R.restatement(i, mutant)
    return i, ref, rest, R.candidate(cand)


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_equals_float64_autograd(name):
    i = R.make_inputs(name)
    c = i.case
    ref = R.reference(i)
    d = torch.float64
    _, S = R.stream(i)
    S.requires_grad_(True)
    w, b = i.w.to(d).requires_grad_(True), i.b.to(d).requires_grad_(True)
    y = F.layer_norm(S, (c.cols,), w, b, c.eps)
    leaves = [S, w, b]
    if i.gamma is not None:
        gam, bet = i.gamma.to(d).requires_grad_(True), i.beta.to(d).requires_grad_(True)
        y = gam.repeat_interleave(c.rpg, 0) * y + bet.repeat_interleave(c.rpg, 0)
        leaves += [gam, bet]
    loss = (S * 0).sum()
    if i.dy is not None:
        loss = loss + (y * i.dy.to(d)).sum()
    if i.dsum is not None:
        loss = loss + (S * i.dsum.to(d)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    var, mean = torch.var_mean(S.detach(), -1, unbiased=False)
    want = dict(zip(("dx", "dw", "db", "dgamma", "dbeta"), grads), y=y.detach(), mean=mean,
                rstd=(var + c.eps).rsqrt())
    for k, t in want.items():
        t = torch.zeros_like(ref[k]) if t is None else t
        err, scale = (ref[k] - t).abs().max().item(), t.abs().max().item()
        assert err <= 1e-12 * scale, f"{k}: {err:.3e} against max {scale:.3e}"
    if c.res:
        assert torch.equal(ref["dres"], ref["dx"])
        exact = i.x.double() + i.res.double()
        assert torch.equal(ref["x_sum"], exact)
        if c.io == R.BF16:          # the leaf is the stored value, one rounding from the exact sum
            assert torch.equal(S.detach(), S.detach().bfloat16().double())
            assert ((S.detach() - exact).abs() <= R.BF16_ULP * exact.abs()).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_passes_the_criterion(name):
    i, ref, rest, cand = _run(name)
    ratios = R.check(cand, ref, rest, i.case.io, name)
    for k in ("y", "dx", "dw", "db"):
        assert k in ratios
    # a float32 tensor of the restatement is its own yardstick
    assert all(q in (0.0, 1.0) or cand[k].dtype == R.BF16 or k == "dx_colsum" for k, (q, _) in ratios.items()), ratios


KILLS = {
    "var_n_minus_1": ["vec-f32-2048", "vec-f32-512", "scalar-f32-64", "vec-bf16-4096"],
    "eps_outside_sqrt": ["num-small-1e-05-f32", "num-small-1e-06-f32", "num-small-1e-05-bf16"],
    "eps_dropped": ["num-small-1e-05-f32", "num-small-1e-06-f32", "num-const_row-1e-05-f32",
                    "num-const_row-1e-06-bf16"],
    "dx_no_xhat_term": ["vec-f32-256", "vec-bf16-512", "rows-f32-1"],
    "dgamma_no_bias_term": ["film-128-5x17-f32-f32", "film-1024-3x1-bf16-bf16"],
    "film_group_per_64_rows": ["film-128-5x17-f32-f32", "film-1024-4x96-bf16-bf16", "film-128-7x2-bf16-f32"],
    "ragged_block_dropped": ["vec-f32-256", "rows-f32-4097", "rows-bf16-16385", "wave4-bf16-4096"],
    "colsum_before_rounding": ["vec-bf16-512", "rows-bf16-2049", "film-1024-2x192-bf16-f32"],
}


def test_every_listed_mutant_has_its_cases():
    assert set(KILLS) == set(R.MUTANTS)
    assert all(n in R.BY_NAME for names in KILLS.values() for n in names)


@pytest.mark.parametrize("mutant,name", [(m, n) for m, names in KILLS.items() for n in names])
def test_mutant_misses_the_criterion(mutant, name):
    i, ref, rest, cand = _run(name, mutant)
    errs = R.errors(cand, ref, rest, i.case.io)
    print(mutant, name, {k: f"{e[0]:.2e}" for k, e in errs.items() if e[0] > 0})
    with pytest.raises(AssertionError):
        R.check(cand, ref, rest, i.case.io, name)
    R.check(R.candidate(rest), ref, rest, i.case.io, name)


def test_mutants_that_need_a_shape_leave_the_others_alone():
    """The per-64-row FiLM group is right when rows_per_group % 64 == 0, and
    a block-dropping backward is right when the rows fill their blocks."""
    for mutant, name in (("film_group_per_64_rows", "film-128-3x64-f32-f32"),
                         ("film_group_per_64_rows", "film-1024-2x192-bf16-bf16"),
                         ("ragged_block_dropped", "rows-f32-8")):
        i, ref, rest, cand = _run(name, mutant)
        R.check(cand, ref, rest, i.case.io, name)


def test_earlier_bounds_passed_these_mutants():
    """Why the criterion changed: 1e-3 of the maximum (fp32) lets the n - 1
    variance through at cols >= 1024, and both eps mutants on unit-variance rows."""
    rel = lambda a, b: (a.double() - b).abs().max().item() / b.abs().max().item()
    for name in ("vec-f32-1024", "vec-f32-2048"):
        i, ref, rest, cand = _run(name, "var_n_minus_1")
        assert all(rel(cand[k], ref[k]) < 1e-3 for k in ("y", "dx", "dw", "db")), name
    for mutant in ("eps_outside_sqrt", "eps_dropped"):
        i, ref, rest, cand = _run("vec-f32-1024", mutant)
        assert all(rel(cand[k], ref[k]) < 1e-4 for k in ("y", "dx", "dw", "db")), mutant
        with pytest.raises(AssertionError):
            R.check(cand, ref, rest, i.case.io)


def test_check_rejects_nan_and_a_wrong_dtype():
    i, ref, rest, cand = _run("vec-f32-256")
    bad = dict(cand, dx=cand["dx"].clone())
    bad["dx"][5, 7] = float("nan")
    with pytest.raises(AssertionError):
        R.check(bad, ref, rest, i.case.io)
    with pytest.raises(AssertionError):
        R.check(dict(cand, y=cand["y"].bfloat16()), ref, rest, i.case.io)
    # a bf16 tensor gets one rounding of its own element and no more
    i, ref, rest, cand = _run("vec-bf16-512")
    y = cand["y"].clone()
    k = ref["y"].abs().argmax()
    y.view(-1)[k] = (ref["y"].view(-1)[k] * (1 + 3 * R.BF16_ULP)).bfloat16()
    with pytest.raises(AssertionError):
        R.check(dict(cand, y=y), ref, rest, i.case.io)


def test_row_block_is_ln_rb():
    assert [R.row_block(r) for r in (1, 37, 2049, 4097, 8193, 16385)] == [8, 8, 8, 16, 32, 64]
    assert [R.row_block(G * rpg, rpg) for G, rpg in ((3, 1), (7, 2), (5, 17), (4, 96), (3, 64), (2, 192), (1, 40),
                                                     (2, 19))] == [1, 2, 1, 32, 64, 64, 8, 1]


def test_case_list_covers_the_dispatch():
    """13 column cases x the dtypes that reach them, and all four T / TG pairs."""
    vec = {(c.io, c.cols // (64 * (4 if c.io == R.F32 else 8))) for c in R.CASES if c.name.startswith("vec-")}
    assert vec == {(io, nv) for io in (R.F32, R.BF16) for nv in (1, 2, 3, 4, 6, 8)}
    scalar = {(c.io, c.cols // 64) for c in R.CASES if c.name.startswith(("scalar-", "forced-"))}
    assert {nv for io, nv in scalar if io == R.F32} == {1, 2, 3, 4, 6, 8, 16}
    assert {nv for io, nv in scalar if io == R.BF16} == {1, 2, 3, 4, 6, 8, 16}
    assert {(c.io, c.gb) for c in R.CASES if c.name.startswith("film-")} == {(a, b) for a in (R.F32, R.BF16)
                                                                              for b in (R.F32, R.BF16)}
