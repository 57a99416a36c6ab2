"""linear.param_grads, the one owner of a projection parameter's weight and
bias gradients (row-slice parts, zero fill of uncovered rows, BiasGradSlot,
immediate or deferred), called directly against an fp64 reference and through
CrossAttention's four in-projection paths and KVAllFn.

Width 256 is the smallest wgrad._eligible admits; 128 tokens take the TN
kernel, 96 (no multiple of 64) torch's product in linear.wgrad.  fp32 sums of
exact bf16 products in different orders agree to 1e-4 of each tensor's scale
(test_gpu_wgrad._check, the project's figure for this comparison)."""
import pytest
import torch

from test_gpu_ops import close, DEV
from test_gpu_wgrad import _check

pytestmark = pytest.mark.gpu

D, H = 256, 4
TOL = 1e-4
PART_SETS = [None, [(0, D)], [(0, D), (D, 3 * D)], [(2 * D, 3 * D)], [(0, D), (2 * D, 3 * D)]]


@pytest.fixture(scope="module")
def operands():
    """Per token count M: dy (M, 3d) and two x (M, d) in bf16 on the device
    (part i of a set reads x[i]), with the fp64 products dy^T x[i] and the
    fp64 column sums of dy, computed once on the CPU."""
    out = {}
    g = torch.Generator().manual_seed(3)
    for M in (128, 96):
        dy = torch.randn(M, 3 * D, generator=g).bfloat16()
        xs = [torch.randn(M, D, generator=g).bfloat16() for _ in range(2)]
        out[M] = (dy.to(DEV), [x.to(DEV) for x in xs], [dy.double().t() @ x.double() for x in xs], dy.double().sum(0))
    return out


def _params():
    return torch.empty(3 * D, D, device=DEV), torch.empty(3 * D, device=DEV)


def _parts(dy, xs, rows):
    if rows is None:
        return [(dy, xs[0], None)]
    return [(dy[:, r0:r1].contiguous(), xs[i], (r0, r1)) for i, (r0, r1) in enumerate(rows)]


def _expected(refs_w, ref_b, rows):
    """The full fp64 gradients: the parts' rows, zero elsewhere."""
    eW, eb = torch.zeros(3 * D, D, dtype=torch.float64), torch.zeros(3 * D, dtype=torch.float64)
    for i, (r0, r1) in enumerate(rows or [(0, 3 * D)]):
        eW[r0:r1], eb[r0:r1] = refs_w[i][r0:r1], ref_b[r0:r1]
    return eW, eb


@pytest.mark.parametrize("M", [128, 96])
@pytest.mark.parametrize("rows", PART_SETS, ids=lambda r: "whole" if r is None else "+".join(f"{a}:{b}" for a, b in r))
def test_immediate_parts_against_fp64(operands, M, rows):
    from mtts.linear import param_grads
    dy, xs, refs_w, ref_b = operands[M]
    W, b = _params()
    parts = _parts(dy, xs, rows)
    # best effort: leave NaNs in the block the allocator is likely to hand out next
    stale = torch.full((3 * D, D), float("nan"), device=DEV)
    del stale
    dW, db = param_grads(W, b, parts, True, True)
    assert dW.dtype == W.dtype and db.dtype == b.dtype
    assert dW.shape == W.shape and db.shape == b.shape
    eW, eb = _expected(refs_w, ref_b, rows)
    covered = torch.zeros(3 * D, dtype=torch.bool)
    for r0, r1 in rows or [(0, 3 * D)]:
        covered[r0:r1] = True
    dWc, dbc = dW.cpu(), db.cpu()
    for name, got, ref in (("dW", dWc, eW), ("db", dbc, eb)):
        err = (got[covered].double() - ref[covered]).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{name} M={M} rows={rows}: err {err:.3e} scale {scale:.3e}")
        assert torch.isfinite(got[covered]).all() and err <= TOL * scale, f"{name}: {err:.3e} > {TOL} * {scale:.3e}"
        assert torch.count_nonzero(got[~covered]) == 0, f"{name}: uncovered rows not exactly zero"
    # need_w / need_b off: nothing is computed
    assert param_grads(W, b, parts, False, False) == (None, None)


def test_overlapping_parts_raise(operands):
    from mtts.linear import param_grads
    dy, xs, _, _ = operands[128]
    W, b = _params()
    with pytest.raises(ValueError):
        param_grads(W, b, _parts(dy, xs, [(0, D), (D // 2, D // 2 + D)]), True, True)
    with pytest.raises(ValueError):
        param_grads(W, b, [(dy, xs[0], None), (dy[:, :D].contiguous(), xs[1], (0, D))], True, True)


@pytest.mark.parametrize("rows", [None, [(D, 2 * D)]], ids=["whole", "slice"])
def test_bias_slot_taken_or_ignored(operands, rows):
    """A slot value of the part's length is consumed and returned (in the
    part's rows); one of another length is dropped and the column sum taken."""
    from mtts.linear import BiasGradSlot, param_grads
    dy, xs, refs_w, ref_b = operands[128]
    W, b = _params()
    parts = _parts(dy, xs, rows)
    r0, r1 = rows[0] if rows else (0, 3 * D)
    slot = BiasGradSlot()
    slot.value = torch.arange(1, r1 - r0 + 1, device=DEV, dtype=torch.float32)
    _, db = param_grads(W, b, parts, False, True, slot)
    assert slot.value is None
    assert torch.equal(db[r0:r1], torch.arange(1, r1 - r0 + 1, device=DEV, dtype=torch.float32))
    assert torch.count_nonzero(db) == r1 - r0
    slot.value = torch.ones(r1 - r0 + 8, device=DEV)
    _, db = param_grads(W, b, parts, False, True, slot)
    assert slot.value is None
    eb = _expected(refs_w, ref_b, rows)[1]
    close(db, eb, rtol=TOL, name="db from colsum")


# ---------------------------------------------------------------- through CrossAttention

B, TQ, TKV = 2, 128, 64


@pytest.fixture()
def grouped_always(monkeypatch):
    from mtts import wgrad
    monkeypatch.setattr(wgrad, "MIN_GROUP_TILES", 0)   # as test_gpu_wgrad: these flushes hold few tiles
    return wgrad


def _attn(n=1, seed=0):
    from mtts.attention import CrossAttention
    torch.manual_seed(seed)
    mods = [CrossAttention(D, H).to(DEV) for _ in range(n)]
    for m in mods:
        torch.nn.init.normal_(m.in_proj_bias, std=0.1)
    return mods


def _inputs(tkv=TKV, seed=1):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, TQ, D, generator=g).to(DEV).bfloat16()
    k = torch.randn(B, tkv, D, generator=g).to(DEV).bfloat16()
    v = torch.randn(B, tkv, D, generator=g).to(DEV).bfloat16()
    w = torch.randn(B, TQ, D, generator=g).to(DEV)
    return q, k, v, w


def _both_modes(wgrad, mods, loss_fn):
    """{deferred: {name: grad}} of one backward without and one with wgrad.deferred()."""
    out = {}
    for defer in (False, True):
        for m in mods:
            m.zero_grad(set_to_none=True)
        with wgrad.deferred(defer):
            loss_fn().backward()
        assert not wgrad._E.jobs
        out[defer] = {f"{i}.{n}": p.grad.detach().clone() for i, m in enumerate(mods)
                      for n, p in m.named_parameters() if p.grad is not None}
    return out


@pytest.mark.parametrize("path", ["key_is_value", "separate_kv"])
def test_cross_attention_immediate_equals_deferred(grouped_always, path):
    """InProjFn (key is value: q + kv parts) and three row-sliced LinearFns."""
    (att,) = _attn()
    q, k, v, w = _inputs()
    if path == "key_is_value":
        v = k
    out = _both_modes(grouped_always, [att], lambda: (att(q, k, v)[0].float() * w).sum())
    assert set(out[True]) == {"0.in_proj_weight", "0.in_proj_bias", "0.out_proj.weight", "0.out_proj.bias"}
    assert out[True]["0.in_proj_weight"].abs().max() > 0
    _check(out[True], out[False])


def test_single_key_gives_only_value_rows(grouped_always):
    """One unmasked key: only the value projection runs (rows 2d:3d of
    in_proj); rows 0:2d of both gradients are exactly zero in both modes."""
    (att,) = _attn()
    q, k, v, w = _inputs(tkv=1)
    out = _both_modes(grouped_always, [att], lambda: (att(q, k, v)[0].float() * w).sum())
    for mode in out.values():
        for n in ("0.in_proj_weight", "0.in_proj_bias"):
            assert torch.count_nonzero(mode[n][:2 * D]) == 0, n
            assert mode[n][2 * D:].abs().max() > 0, n
    _check(out[True], out[False])


def test_kv_all_with_an_unused_layer(grouped_always):
    """kv_all over three modules, the middle one's output unused: its K/V
    gradient never arrives, KVAllFn assembles the operand and produces that
    layer's rows d:3d itself -- exact zeros, as rows 0:d no part covers -- in
    both modes.  The used layers equal their own per-layer projections
    (InProjFn) to 3e-2: the K/V activations are bf16 outputs of two different
    GEMM shapes, the bound test_gpu_kvall.py sets for that comparison."""
    from mtts.attention import kv_all, kv_all_ok
    mods = _attn(3)
    q, k, _, w = _inputs()
    assert kv_all_ok(k, mods)

    def batched():
        kvs = kv_all(k, mods)
        return sum((mods[l](q, k, k, _kv=kvs[l])[0].float() * w).sum() for l in (0, 2))
    out = _both_modes(grouped_always, mods, batched)
    for mode in out.values():
        assert set(mode) == {f"{l}.{n}" for l in (0, 2) for n, _ in mods[0].named_parameters()} | \
            {"1.in_proj_weight", "1.in_proj_bias"}
        assert torch.count_nonzero(mode["1.in_proj_weight"]) == 0
        assert torch.count_nonzero(mode["1.in_proj_bias"]) == 0
    _check(out[True], out[False])
    ref = _both_modes(grouped_always, mods, lambda: sum((mods[l](q, k, k)[0].float() * w).sum() for l in (0, 2)))
    for n, g in ref[False].items():
        close(out[False][n], g, rtol=3e-2, name=n)


def test_kv_view_with_a_second_consumer_raises(grouped_always):
    """A layer's K/V view that also feeds something besides its attention: its
    q projection has already produced in_proj rows d:3d from the attention's
    dK / dV alone, so KVAllFn refuses the backward instead of dropping the
    other contribution; the engine is left empty."""
    from mtts.attention import kv_all
    wgrad = grouped_always
    mods = _attn(2)
    q, k, _, w = _inputs()
    kvs = kv_all(k, mods)
    loss = sum((mods[l](q, k, k, _kv=kvs[l])[0].float() * w).sum() for l in (0, 1)) + kvs[1].float().sum()
    with pytest.raises(RuntimeError, match=r"layer 1\b"):
        with wgrad.deferred():
            loss.backward()
    assert not wgrad._E.jobs and not wgrad._E.callback_queued
