"""The split-key single-query attention (mtts_attention_decode_split,
csrc/attn.hip attn_decode_split_kernel + attn_decode_merge_kernel) against the
float64 reference of tests/test_gpu_attention.py, a row's reference computed
on its first kv_lens[b] keys only.  Bounds: 2e-5 (fp32) / 2e-2 (bf16) of the
output scale, as that file's; lse at 1e-5 in both dtypes (an fp32 output
accumulated in fp32 from the very bf16 inputs the reference reads).  Everything a
row's bits may depend on is the row itself: exact comparisons across batch
sizes, row positions, layouts, output forms and what lies past its count."""
import pytest
import torch

from test_gpu_attention import close, make, ref_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 128), (2, 64), (4, 16)]                      # (H, hd)


def _ck(hd):
    from mtts.attn_kernels import decode_split_chunk
    return decode_split_chunk(hd)


def _split(q, kv, H, kpm=None, lens=None, **kw):
    from mtts.attn_kernels import attention_decode_split
    d = q.shape[-1]
    n = None if lens is None else torch.as_tensor(lens, dtype=torch.int32).to(DEV)
    return attention_decode_split(q[:, 0], kv[..., :d], kv[..., d:], H, kpm, n, **kw)


def _check_rows(out, lse, q, kv, H, kpm, lens, dtype, rows=None):
    """Every row in `rows` against the reference on its first lens[b] keys."""
    d = q.shape[-1]
    tol, ltol = (2e-5 if dtype == torch.float32 else 2e-2), 1e-5
    for b in (range(q.shape[0]) if rows is None else rows):
        n = kv.shape[1] if lens is None else min(lens[b], kv.shape[1])
        m = None if kpm is None else kpm[b:b + 1, :n]
        ref, ref_lse = ref_attention(q[b:b + 1], kv[b:b + 1, :n, :d], kv[b:b + 1, :n, d:], H, m)
        close(out[b:b + 1, None], ref, tol)
        if lse is not None:
            close(lse[b:b + 1, :, None], ref_lse, ltol)


def _sizes(hd):
    ck = _ck(hd)
    return [5, ck, ck + 1, 2 * ck, 2 * ck + 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_parity_at_the_chunk_edges(H, hd, dtype):
    ck = _ck(hd)
    for S in _sizes(hd):
        q, kv, kpm = make(5, 1, S, H, hd, dtype, seed=S % 97)
        lens = [1, ck, ck + 1, S, min(7, S)]                # a count past S means S: the kernel clamps it
        out, lse = _split(q, kv, H, kpm, lens, want_lse=True)
        assert out.shape == (5, H * hd) and out.dtype == dtype and lse.shape == (5, H)
        _check_rows(out, lse, q, kv, H, kpm, lens, dtype)
        out, lse = _split(q, kv, H, kpm, None, want_lse=True)
        _check_rows(out, lse, q, kv, H, kpm, None, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_keys_past_the_count_do_not_reach_the_result(H, hd, dtype):
    ck = _ck(hd)
    S = 2 * ck + 3
    q, kv, kpm = make(5, 1, S, H, hd, dtype, seed=5)
    lens = [1, ck, ck + 1, S, 7]
    clean, clean_lse = _split(q, kv, H, kpm, lens, want_lse=True)
    dirty, mask = kv.clone(), kpm.clone()
    for b, n in enumerate(lens):
        dirty[b, n:] = float("nan")
        mask[b, n:] = False                                 # only the count keeps them out
    got, got_lse = _split(q, dirty, H, mask, lens, want_lse=True)
    assert torch.isfinite(got.float()).all() and torch.isfinite(got_lse).all()
    assert torch.equal(got, clean) and torch.equal(got_lse, clean_lse)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_a_count_is_a_mask(H, hd, dtype):
    ck = _ck(hd)
    S = 2 * ck + 3
    q, kv, _ = make(3, 1, S, H, hd, dtype, seed=6, mask=False)
    lens = [1, ck, ck + 1]
    by_count, lse_c = _split(q, kv, H, None, lens, want_lse=True)
    kpm = torch.arange(S, device=DEV)[None, :] >= torch.tensor(lens, device=DEV)[:, None]
    by_mask, lse_m = _split(q, kv, H, kpm, None, want_lse=True)
    assert torch.equal(by_count, by_mask) and torch.equal(lse_c, lse_m)
    _check_rows(by_count, lse_c, q, kv, H, None, lens, dtype)
    # a chunk in the middle of the range with every key masked
    S3 = 3 * ck
    q, kv, kpm = make(2, 1, S3, H, hd, dtype, seed=7)
    kpm[0, ck:2 * ck] = True
    lens = [S3, S3 - 2]
    out, lse = _split(q, kv, H, kpm, lens, want_lse=True)
    _check_rows(out, lse, q, kv, H, kpm, lens, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_empty_and_fully_masked_rows(H, hd, dtype):
    ck = _ck(hd)
    S = ck + 9
    q, kv, kpm = make(4, 1, S, H, hd, dtype, seed=8)
    lens = [S, 0, ck + 1, S]
    kpm[3] = True                                           # every key masked
    out, lse = _split(q, kv, H, kpm, lens, want_lse=True)
    for b in (1, 3):
        assert torch.isnan(out[b].float()).all(), b
        assert (lse[b] == float("-inf")).all(), b
    _check_rows(out, lse, q, kv, H, kpm, lens, dtype, rows=(0, 2))
    # the packed image of such a row is NaN as well, and its neighbours are untouched
    if dtype == torch.bfloat16:
        img = _split(q, kv, H, kpm, lens, packed=True).unpack()
        assert torch.isnan(img[1].float()).all() and torch.equal(img[0], out[0]) and torch.equal(img[2], out[2])


@pytest.mark.parametrize("H,hd", SHAPES)
def test_a_row_does_not_depend_on_its_company(H, hd):
    ck = _ck(hd)
    S = 2 * ck + 3
    dtype = torch.bfloat16
    q, kv, kpm = make(20, 1, S, H, hd, dtype, seed=9)
    n = ck + 5
    alone = _split(q[:1], kv[:1], H, kpm[:1], [n])
    alone_img = _split(q[:1], kv[:1], H, kpm[:1], [n], packed=True).unpack()
    assert torch.equal(alone_img, alone)

    def among(B, at, lens):
        idx = list(range(1, B))
        idx.insert(at, 0)                                   # row 0 of the data at position `at`
        lens = list(lens)
        lens[at] = n
        return idx, lens

    idx, lens = among(5, 3, [S, 1, ck, 0, 2 * ck + 1])
    got = _split(q[idx], kv[idx], H, kpm[idx], lens)
    assert torch.equal(got[3:4], alone)
    idx, lens = among(20, 17, [1 + (37 * i) % S for i in range(20)])
    got = _split(q[idx], kv[idx], H, kpm[idx], lens, packed=True).unpack()
    assert torch.equal(got[17:18], alone)
    # and not on the key side's padded length either: the same row inside a longer buffer
    longer = torch.cat([kv[:1], torch.full_like(kv[:1, :ck], float("nan"))], 1)
    mask = torch.cat([kpm[:1], torch.zeros(1, ck, dtype=torch.bool, device=DEV)], 1)
    assert torch.equal(_split(q[:1], longer, H, mask, [n]), alone)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_layouts_and_output_forms_agree(H, hd, dtype):
    from mtts.attn_kernels import attention_decode_split
    ck = _ck(hd)
    S = 2 * ck + 3
    B, d = 3, H * hd
    q, kv, kpm = make(B, 1, S, H, hd, dtype, seed=10)
    lens = torch.tensor([S, ck + 1, 9], dtype=torch.int32, device=DEV)
    k, v = kv[..., :d], kv[..., d:]
    row, lse = attention_decode_split(q[:, 0], k, v, H, kpm, lens, want_lse=True)
    khm = k.reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()
    vhm = v.reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()
    hm, lse_hm = attention_decode_split(q[:, 0], khm, vhm, H, kpm, lens, want_lse=True)
    assert torch.equal(hm, row) and torch.equal(lse_hm, lse)
    if dtype == torch.bfloat16:
        for kk, vv in ((k, v), (khm, vhm)):
            img = attention_decode_split(q[:, 0], kk, vv, H, kpm, lens, packed=True)
            assert torch.equal(img.unpack(), row)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_one_chunk_is_the_single_pass_kernel(H, hd, dtype):
    """A key side of at most one chunk gives the same bits through the split
    path and through the single-pass kernel (csrc/attn.hip decode_single_pass
    is the body of both; the merge of one chunk multiplies by exp2(0) and adds
    to zero; the U = 4 and U = 8 forms put key j in the same group at the same
    u, and the extra u add p = 0 times a finite clamped key)."""
    from mtts.attn_kernels import attention_decode_packed, attention_decode_split, attention_fwd
    B, d, ng = 3, H * hd, 256 // (hd // 8)
    assert 8 * ng == _ck(hd)
    for S in (5, 4 * ng, 4 * ng + 1, 8 * ng):               # the U = 4 edge, the first key of U = 8, a full chunk
        q, kv, kpm = make(B, 1, S, H, hd, dtype, seed=11 + S % 89)      # the mask leaves every row key 0
        k, v = kv[..., :d], kv[..., d:]
        out, lse = attention_decode_split(q[:, 0], k, v, H, kpm, None, want_lse=True)
        one, one_lse = attention_fwd(q, k, v, H, kpm, want_lse=True)
        assert torch.equal(out, one[:, 0]) and torch.equal(lse, one_lse[:, :, 0]), S
        if dtype == torch.bfloat16:
            khm = k.reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()
            vhm = v.reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()
            for kk, vv in ((k, v), (khm, vhm)):
                img = attention_decode_split(q[:, 0], kk, vv, H, kpm, None, packed=True)
                assert torch.equal(attention_decode_packed(q[:, 0], kk, vv, H, kpm).unpack(), img.unpack()), S


def _args(B, H, hd, S, dtype, packed=False):
    from mtts import _lib as L
    from mtts.attn_kernels import _fwd_args
    from mtts.ops import PackedAct
    d = H * hd
    q = torch.zeros(B, 1, d, device=DEV, dtype=dtype)
    kv = torch.zeros(B, S, 2 * d, device=DEV, dtype=dtype)
    out = torch.empty(B, 1, d, device=DEV, dtype=dtype)
    a = L.AttnDecodeSplitArgs()
    a.f = _fwd_args(q, kv[..., :d], kv[..., d:], H, None, out, None)
    n = L.lib().mtts_attention_decode_split_workspace(B, H, hd, S)
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), n
    keep = [q, kv, out, ws]
    if packed:
        keep.append(PackedAct.empty(B, d, DEV))
        a.f.out_packed = keep[-1].data.data_ptr()
    return a, keep


def test_c_abi_refusals_name_the_argument():
    from mtts import _lib as L
    a, keep = _args(2, 2, 64, 300, torch.bfloat16)
    L.call("mtts_attention_decode_split", a)                # the arguments as built are accepted
    a.f.q_len = 2
    with pytest.raises(RuntimeError, match="q_len 2"):
        L.call("mtts_attention_decode_split", a)
    a, keep = _args(2, 2, 64, 300, torch.bfloat16)
    a.workspace_bytes -= 1
    with pytest.raises(RuntimeError, match="workspace"):
        L.call("mtts_attention_decode_split", a)
    a, keep = _args(2, 2, 64, 300, torch.float32, packed=True)
    with pytest.raises(RuntimeError, match="out_packed"):
        L.call("mtts_attention_decode_split", a)
    a, keep = _args(32, 2, 64, 300, torch.bfloat16, packed=True)
    L.call("mtts_attention_decode_split", a)                # 32 rows: the whole image
    a.f.batch = 33
    with pytest.raises(RuntimeError, match="out_packed"):
        L.call("mtts_attention_decode_split", a)
    a, keep = _args(2, 2, 64, 300, torch.bfloat16)
    a.f.out = None
    with pytest.raises(RuntimeError, match="out and out_packed"):
        L.call("mtts_attention_decode_split", a)
    torch.cuda.synchronize()
