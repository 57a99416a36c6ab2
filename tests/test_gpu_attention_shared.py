"""The split-key single-query attention with a K/V row per query row
(mtts_attention_decode_split_shared, csrc/attn.hip
attn_decode_split_shared_kernel + attn_decode_merge_shared_kernel;
attention_decode_split(kv_rows=...)).  The reference is the existing
attention_decode_split on gathered operands, k[kv_rows], v[kv_rows],
kpm[kv_rows], kv_lens[kv_rows], and every comparison is exact: a row's bits do
not depend on whether it read its own copy of the keys or its class's one row.
The partial workspace is filled with NaN before every call, so a partial that
the merge reads and no workgroup wrote shows in the result."""
import pytest
import torch

from test_gpu_attention import make

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 2
ROWS = [2, 0, 2, 2, 0]      # R = 3: K/V row 1 unused, class 2 led by row 0, class 0 led by row 1


def _ck(hd):
    from mtts.attn_kernels import decode_split_chunk
    return decode_split_chunk(hd)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _nan_ws(B, hd, S):
    from mtts.attn_kernels import decode_split_workspace
    n = decode_split_workspace(B, H, hd, S)
    return torch.full((n // 4,), float("nan"), device=DEV, dtype=torch.float32).view(torch.uint8)


def _call(q, k, v, kpm, lens, hd, kv_rows=None, **kw):
    from mtts.attn_kernels import attention_decode_split
    S = k.shape[-2]
    return attention_decode_split(q, k, v, H, kpm, lens, workspace=_nan_ws(q.shape[0], hd, S), kv_rows=kv_rows, **kw)


def _same(a, b):
    """Equal bits where neither is NaN, and NaN in the same places."""
    a, b = a.float(), b.float()
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _head_major(t, hd):
    R, S, _ = t.shape
    return t.reshape(R, S, H, hd).permute(0, 2, 1, 3).contiguous()


def _operands(hd, dtype, B, R, seed):
    """q (B, d); k, v (R, S, d) at S = 2 chunks + 3; a mask with masked keys
    inside every count and every key of chunk 0 of K/V row 0 masked; counts
    [S, 7, chunk + 1] (row 2 stops inside chunk 1 and skips chunk 2)."""
    ck, d = _ck(hd), H * hd
    S = 2 * ck + 3
    q = make(B, 1, S, H, hd, dtype, seed=seed)[0][:, 0]
    _, kv, kpm = make(R, 1, S, H, hd, dtype, seed=seed + 1)
    kpm[0, :ck] = True
    return q, kv[..., :d], kv[..., d:], kpm, _i32([S, 7, ck + 1][:R]), S


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_shared_rows_equal_gathered_copies(hd, dtype):
    q, k, v, kpm, lens, S = _operands(hd, dtype, 5, 3, seed=hd)
    rows = _i32(ROWS)
    idx = rows.long()
    k, v = k.clone(), v.clone()
    k[1], v[1] = float("nan"), float("nan")                 # the unused K/V row is never read
    kg, vg = k[idx], v[idx]
    ref, ref_lse = _call(q, kg, vg, kpm[idx], lens[idx], hd, want_lse=True)
    assert torch.isfinite(ref.float()).all()
    for layout in ("channel-last", "head-major"):
        kk, vv = (k, v) if layout == "channel-last" else (_head_major(k, hd), _head_major(v, hd))
        got, lse = _call(q, kk, vv, kpm, lens, hd, kv_rows=rows, want_lse=True)
        assert torch.equal(got, ref) and torch.equal(lse, ref_lse), layout
        if dtype == torch.bfloat16:
            img = _call(q, kk, vv, kpm, lens, hd, kv_rows=rows, packed=True)
            assert torch.equal(img.unpack(), ref), layout
            kr, vr = (kg, vg) if layout == "channel-last" else (_head_major(kg, hd), _head_major(vg, hd))
            assert torch.equal(img.unpack(), _call(q, kr, vr, kpm[idx], lens[idx], hd, packed=True).unpack()), layout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_identity_rows_equal_the_plain_call(hd, dtype):
    q, k, v, kpm, lens, S = _operands(hd, dtype, 3, 3, seed=3 + hd)
    ref, ref_lse = _call(q, k, v, kpm, lens, hd, want_lse=True)
    got, lse = _call(q, k, v, kpm, lens, hd, kv_rows=_i32([0, 1, 2]), want_lse=True)
    assert torch.equal(got, ref) and torch.equal(lse, ref_lse)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_33_rows_in_one_class(hd, dtype):
    q, k, v, kpm, lens, S = _operands(hd, dtype, 33, 2, seed=7 + hd)
    lens = _i32([S, S])
    kpm[1, :_ck(hd)] = True                                 # chunk 0 of the one row read: a partial of -inf, 0, zeros
    kpm[1, _ck(hd)] = False
    rows = torch.ones(33, dtype=torch.int32, device=DEV)
    idx = rows.long()
    ref, ref_lse = _call(q, k[idx], v[idx], kpm[idx], lens[idx], hd, want_lse=True)
    got, lse = _call(q, k, v, kpm, lens, hd, kv_rows=rows, want_lse=True)
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got, ref) and torch.equal(lse, ref_lse)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_rows_outside_the_kv_batch_have_no_keys(hd, dtype):
    q, k, v, kpm, lens, S = _operands(hd, dtype, 5, 3, seed=11 + hd)
    rows = _i32([2, -1, 2, 3, 0])                           # -1 and R
    idx = torch.tensor([2, 0, 2, 0, 0], device=DEV)
    glens = lens[idx].clone()
    glens[1], glens[3] = 0, 0                               # what a zero-key row gives today
    ref, ref_lse = _call(q, k[idx], v[idx], kpm[idx], glens, hd, want_lse=True)
    got, lse = _call(q, k, v, kpm, lens, hd, kv_rows=rows, want_lse=True)
    assert ref[[1, 3]].isnan().all() and torch.isfinite(ref[[0, 2, 4]].float()).all()
    assert _same(got, ref) and torch.equal(lse, ref_lse)
    if dtype == torch.bfloat16:
        img = _call(q, k, v, kpm, lens, hd, kv_rows=rows, packed=True)
        assert _same(img.unpack(), ref)


def test_argument_checks():
    hd = 64
    q, k, v, kpm, lens, S = _operands(hd, torch.bfloat16, 5, 3, seed=1)
    with pytest.raises(ValueError, match="kv_rows"):
        _call(q, k, v, kpm, lens, hd, kv_rows=torch.tensor(ROWS, device=DEV))          # int64
    with pytest.raises(ValueError, match="kv_rows"):
        _call(q, k, v, kpm, lens, hd, kv_rows=_i32(ROWS[:4]))
    with pytest.raises(ValueError, match="kv_lens"):
        _call(q, k, v, kpm, lens[:2], hd, kv_rows=_i32(ROWS))
    with pytest.raises(ValueError):
        _call(q, k, v, kpm[:2], lens, hd, kv_rows=_i32(ROWS))
    with pytest.raises(ValueError, match="rows"):
        _call(q, k, v, kpm, lens, hd)                       # without kv_rows k / v are per query row
