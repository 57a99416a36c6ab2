"""tests/token_ref.py proven on the CPU: the float64 references against float64
autograd through torch's own cross_entropy and embedding, the float32
restatements of csrc/loss.hip and of the embedding kernels of
csrc/regulate.hip against the criterion on every case the GPU file runs, and
the criterion against the mutants it has to tell from a right kernel.

Each mutant and the first case that rejects it (KILLS lists more), with the
amount by which it misses its bound as a fraction of the tensor's maximum:
    no_max_subtraction           ce-num-plus90-f32     loss, lse: inf where the reference is finite
    mean_over_all_rows           ce-ign-default-f32    loss 2.9e-1, dlogits 2.9e-1, count: bits differ
    ignored_row_has_grad         ce-ign-default-f32    dlogits: non-zero where the reference is exactly 0
    grad_ignores_gout            ce-rows-257x10-f32    dlogits 4.3e-1
    row_stride_is_V              ce-strided-10-f32     loss, lse, dlogits: NaN from outside the slice
    sum_one_trip_only            ce-rows-70000x3-f32   loss 1.2e-3, dlogits 6.9e-2, count: bits differ
    onehot_shifted               ce-rows-257x10-f32    dlogits 1.0
    bf16_truncates               emb-d-64-bf16         y: bits differ
    pos_from_flat_index          emb-codec-5x64-f32    y: bits differ
    bad_row_not_zeroed           emb-bad-64-f32        y: bits differ, non-zero on a zero row
    lane_loop_one_trip           emb-d-260-f32         y: bits differ
    tail_rows_dropped            tg-n-65-f32           out 2.5e-1
    second_column_block_dropped  tg-d-264-f32          out 8.0e-1
    oob_bin_written              tg-ids-live-f32       out 9.4e-1
The nearest mutant is `sum_one_trip_only` on 70 000 x 3 in bf16, where the 18
dropped block partials move the loss by 9.2e-4 of itself (the count, compared
bit for bit, misses those blocks' rows); next is `mean_over_all_rows` with one row
of 257 ignored, 3.9e-3.  The restatements themselves sit at 7e-8 to 3e-7 of a
tensor's maximum (1.4e-5 for the bf16 gradient before its rounding on the
coarse values near 256)."""
import pytest
import torch
import torch.nn.functional as F

import token_ref as R

NAMES = [c.name for c in R.CASES]
CE, EMB, TG = R.names("ce-"), R.names("emb-"), R.names("tg-")


def _close(a, b, what):
    a, b = a.double(), b.double()
    fin = torch.isfinite(b)
    inf = torch.isinf(b)
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[inf], b[inf])
    if fin.any():
        err, scale = (a[fin] - b[fin]).abs().max().item(), b[fin].abs().max().item()
        assert err <= 1e-12 * scale, f"{what}: {err:.3e} against max {scale:.3e}"


@pytest.mark.parametrize("name", [n for n in CE if "-oor-" not in n])
def test_ce_reference_equals_float64_autograd(name):
    i = R.make_inputs(name)
    ref = R.ce_reference(i.x, i.t, i.ignore, i.gout)
    x = i.x.double().requires_grad_(True)
    loss = F.cross_entropy(x, i.t, ignore_index=i.ignore)
    if "-ign-all-" in name:            # torch's mean of no rows is NaN, its gradient 0 / 0; the contract says 0
        assert torch.isnan(loss) and torch.isnan(ref["loss"]) and ref["count"] == 0 and not ref["dlogits"].any()
    else:
        (loss * i.gout).backward()
        _close(ref["loss"], loss.detach(), "loss")
        _close(ref["dlogits"], x.grad, "dlogits")
        assert not ref["dlogits"][i.t == i.ignore].any()
    _close(ref["lse"], torch.logsumexp(i.x.double(), 1), "lse")
    assert ref["count"] == (i.t != i.ignore).sum()


@pytest.mark.parametrize("name", R.names("ce-oor-"))
def test_ce_reference_out_of_range_target(name):
    """Where torch asserts: NaN loss, the rows counted, softmax g / count without a one-hot term."""
    i = R.make_inputs(name)
    ref = R.ce_reference(i.x, i.t, i.ignore, i.gout)
    assert torch.isnan(ref["loss"]) and ref["count"] == (i.t != i.ignore).sum()
    p = torch.softmax(i.x.double(), 1) * (i.gout / ref["count"])
    for r in (17, 280):
        _close(ref["dlogits"][r], p[r], f"row {r}")
    ok = R.ce_reference(i.x, i.t.clamp(0, i.case.V - 1).where(i.t != i.ignore, i.t), i.ignore, i.gout)
    keep = torch.ones(i.case.rows, dtype=torch.bool)
    keep[[17, 280]] = False
    assert torch.equal(ref["dlogits"][keep], ok["dlogits"][keep]) and torch.equal(ref["lse"], ok["lse"])


@pytest.mark.parametrize("name", [n for n in EMB if R.BY_NAME[n].grads])
def test_embed_reference_equals_float64_autograd(name):
    i = R.make_inputs(name)
    ref = R.embed_reference(i)
    tw, qw, pw = (w.double().requires_grad_(True) for w in (i.tw, i.qw, i.pw))
    y = F.embedding(i.tok, tw) + F.embedding(i.qid.long(), qw)[None] + F.embedding(i.pid.long(), pw)[None]
    y.backward(i.dy.double())
    for k, t in (("y", y.detach()), ("d_tok", tw.grad), ("d_quant", qw.grad), ("d_pos", pw.grad)):
        _close(ref[k], t, k)


@pytest.mark.parametrize("name", [n for n in EMB if not R.BY_NAME[n].grads])
def test_embed_reference_zero_fills_bad_rows(name):
    i = R.make_inputs(name)
    c = i.case
    ref = R.embed_reference(i)
    bad = R.bad_rows(i)
    assert int(bad.sum()) == (0 if not c.bad else 3 if c.layout == "at" else 2)
    assert not ref["y"][bad].any()
    pid = i.pid.long() if c.layout == "at" else i.pid.long()[None].expand(c.B, c.L)
    good = ~bad
    want = i.tw.double()[i.tok[good]] + i.qw.double()[i.qid.long()[None].expand(c.B, c.L)[good]] + \
        i.pw.double()[pid[good]]
    assert torch.equal(ref["y"][good], want)


@pytest.mark.parametrize("name", TG)
def test_table_grad_reference_equals_float64_autograd(name):
    i = R.make_inputs(name)
    ref = R.table_grad_reference(i.ids, i.g, i.vocab)["out"]
    ok = (i.ids >= 0) & (i.ids < i.vocab)
    w = torch.zeros(i.vocab, i.case.d, dtype=torch.float64, requires_grad=True)
    F.embedding(i.ids[ok], w).backward(i.g[ok].double())
    _close(ref, w.grad, "out")
    present = torch.zeros(i.vocab, dtype=torch.bool)
    present[i.ids[ok]] = True
    assert not ref[~present].any()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_passes_the_criterion(name):
    i = R.make_inputs(name)
    ref, rest = R.reference(i), R.restatement(i)
    ratios = R.check(R.candidate(rest), ref, rest, i.case.io, name)
    assert set(ratios) == set(ref)
    # a float32 tensor of the restatement is its own yardstick
    assert all(q in (0.0, 1.0) or rest[k].dtype == R.BF16 for k, (q, _) in ratios.items()), ratios


KILLS = {
    "no_max_subtraction": ["ce-num-plus90-f32", "ce-num-plus90-bf16"],
    "mean_over_all_rows": ["ce-ign-default-f32", "ce-ign-block-bf16", "ce-ign-last-f32", "ce-rows-70000x3-f32"],
    "ignored_row_has_grad": ["ce-ign-default-f32", "ce-ign-last-bf16", "ce-ign-all-f32", "ce-ign-block-f32"],
    "grad_ignores_gout": ["ce-rows-257x10-f32", "ce-rows-1x3-bf16", "ce-gout-tensor-f32"],
    "row_stride_is_V": ["ce-strided-10-f32", "ce-strided-10-bf16", "ce-strided-odd-bf16", "ce-codec-bf16"],
    "sum_one_trip_only": ["ce-rows-70000x3-f32", "ce-rows-70000x3-bf16"],
    "onehot_shifted": ["ce-rows-257x10-f32", "ce-rows-37x1024-bf16", "ce-rows-1x3-f32"],
    "bf16_truncates": ["emb-d-64-bf16", "emb-codec-3x129-bf16", "emb-at-bf16"],
    "pos_from_flat_index": ["emb-codec-5x64-f32", "emb-codec-3x129-bf16"],
    "bad_row_not_zeroed": ["emb-bad-64-f32", "emb-bad-260-bf16", "emb-at-bad-f32"],
    "lane_loop_one_trip": ["emb-d-260-f32", "emb-d-260-bf16", "emb-d-512-f32", "emb-d-1024-bf16"],
    "tail_rows_dropped": ["tg-n-65-f32", "tg-n-3-bf16", "tg-n-1-f32", "tg-n-16385-f32", "tg-n-63-bf16"],
    "second_column_block_dropped": ["tg-d-264-f32", "tg-d-520-bf16", "tg-d-1024-bf16", "tg-d-512-f32"],
    "oob_bin_written": ["tg-ids-live-f32", "tg-ids-live-bf16", "tg-n-64-f32"],
}


def test_every_listed_mutant_has_its_cases():
    assert set(KILLS) == set(R.MUTANTS)
    assert all(n in R.BY_NAME for ns in KILLS.values() for n in ns)


@pytest.mark.parametrize("mutant,name", [(m, n) for m, ns in KILLS.items() for n in ns])
def test_mutant_misses_the_criterion(mutant, name):
    i = R.make_inputs(name)
    ref, rest = R.reference(i), R.restatement(i)
    cand = R.candidate(R.restatement(i, mutant))
    errs = R.errors(cand, ref, rest, i.case.io)
    print(mutant, name, {k: f"{e[0]:.2e} ({e[0] / max(ref[k][torch.isfinite(ref[k])].abs().max().item(), 1e-300):.1e})"
                         for k, e in errs.items() if e[0] > 0})
    with pytest.raises(AssertionError):
        R.check(cand, ref, rest, i.case.io, name)
    R.check(R.candidate(rest), ref, rest, i.case.io, name)


def test_mutants_that_need_a_shape_leave_the_others_alone():
    """One trip of ce_sum_kernel is all there is up to 65 536 rows, one lane
    trip up to d = 256, one column block up to 256 fp32 / 512 bf16 columns, no
    tail when n % 4 == 0, and a contiguous tensor's stride is V."""
    for mutant, name in (("sum_one_trip_only", "ce-rows-37x1024-f32"), ("row_stride_is_V", "ce-rows-257x10-bf16"),
                         ("lane_loop_one_trip", "emb-d-256-f32"), ("second_column_block_dropped", "tg-d-256-f32"),
                         ("second_column_block_dropped", "tg-d-512-bf16"), ("tail_rows_dropped", "tg-n-64-f32"),
                         ("oob_bin_written", "tg-vocab16-f32"), ("pos_from_flat_index", "emb-d-64-f32")):
        i = R.make_inputs(name)
        ref, rest = R.reference(i), R.restatement(i)
        R.check(R.candidate(R.restatement(i, mutant)), ref, rest, i.case.io, name)


def test_earlier_bounds_passed_these_mutants():
    """Why the criterion: the earlier bound on a bf16 gradient, 1e-2 of the
    maximum, passes an element two bf16 roundings off; one is all that the
    arithmetic gives."""
    i = R.make_inputs("ce-rows-257x10-bf16")
    ref, rest = R.reference(i), R.restatement(i)
    d = rest["dlogits"].clone()
    k = ref["dlogits"].abs().argmax()
    d.view(-1)[k] = (ref["dlogits"].view(-1)[k] * (1 + 2 * R.BF16_ULP)).bfloat16()       # two roundings off
    assert (d.double() - ref["dlogits"]).abs().max() <= 1e-2 * ref["dlogits"].abs().max()
    with pytest.raises(AssertionError):
        R.check(dict(R.candidate(rest), dlogits=d), ref, rest, R.BF16)


def test_check_rejects_nan_a_wrong_dtype_and_a_moved_infinity():
    i = R.make_inputs("ce-num-tinf-f32")
    ref, rest = R.reference(i), R.restatement(i)
    cand = R.candidate(rest)
    assert torch.isinf(ref["loss"]) and ref["loss"] > 0
    R.check(cand, ref, rest, R.F32)
    for bad in (dict(cand, loss=torch.tensor(R.NAN)), dict(cand, loss=-cand["loss"]),
                dict(cand, loss=torch.tensor(3.0)), dict(cand, dlogits=cand["dlogits"].bfloat16()),
                dict(cand, lse=cand["lse"].index_fill(0, torch.tensor([7]), R.NAN))):
        with pytest.raises(AssertionError):
            R.check(bad, ref, rest, R.F32)
    with pytest.raises(AssertionError):
        R.check(cand, ref, rest, R.BF16)


def test_case_list_covers_the_edges():
    c = R.BY_NAME
    assert {(c[n].rows, c[n].V) for n in R.names("ce-rows-")} == set(R.CE_ROWS)
    assert (70000 + 255) // 256 == 274 and (65536 + 255) // 256 == 256        # the second trip of ce_sum_kernel
    i = R.make_inputs("ce-ign-block-f32")
    assert (i.t[256:512] == 0).all() and (i.t[:256] != 0).all() and (i.t[512:] != 0).all()
    i = R.make_inputs("ce-ign-last-f32")
    assert i.t[-1] == 0 and (i.t[:-1] != 0).all()
    i = R.make_inputs("ce-ign-default-f32")
    assert 0.2 < (i.t == -100).float().mean() < 0.4
    i = R.make_inputs("ce-oor-f32")
    assert i.t[17] == 10 and i.t[280] == -1
    i = R.make_inputs("ce-strided-odd-bf16")
    assert i.x.stride(0) % 2 == 1 and i.x.storage_offset() % 2 == 1
    graph = [int((R.make_inputs(f"ce-graph-{k}-f32").t == 0).sum()) for k in "abc"]
    assert len(set(graph)) == 3
    assert [R.emb_grad_blocks(n) for n in (64, 65, 16384, 16385, 16641, 20000)] == \
        [(64, 1), (64, 2), (64, 256), (68, 241), (68, 245), (80, 250)]
    assert 16641 - 244 * 68 == 49 and 16385 - 240 * 68 == 65          # the last block's rows: 1 mod 4
    assert {R.table_route(c[n]) for n in R.names("tg-route-")} == {"onehot", "index_add"}
    assert all(R.table_route(c[n]) == "hip" for n in R.names("tg-") if "route" not in n)
    i = R.make_inputs("tg-ids-live-f32")
    assert ((i.ids >= 10) & (i.ids < 16)).sum() > 100
