"""FP8 conditioning K/V on the GPU: the quantiser (mtts_kv_quantize_fp8,
csrc/kvq.hip) bit for bit against its CPU definition (tests/kv_fp8_ref.py,
torch's own float8_e4m3fn cast), and the fp8 form of the split-key
single-query attention (mtts_attention_decode_split_fp8) against the float64
reference of tests/test_gpu_attention.py on the dequantised K^ = deq(k8) *
k_scale and V^.  Bounds: that file's and test_gpu_attention_split.py's, 2e-5
(fp32 q) / 2e-2 (bf16 q) of the output scale and 1e-5 for lse -- they transfer
because the kernel accumulates in fp32 from inputs the reference reads exactly.
Everything a row's bits may depend on is the row itself: exact comparisons
across batch sizes, row positions, output forms, workspaces and what lies past
its count."""
import pytest
import torch

from kv_fp8_ref import dequantize_ref, quantize_ref, to_channel_last
from test_gpu_attention import close, ref_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 128), (2, 64), (4, 16)]                      # (H, hd)


def _ck(hd):
    from mtts.attn_kernels import decode_split_chunk
    return decode_split_chunk(hd)


def _i32(v):
    return None if v is None else torch.as_tensor(v, dtype=torch.int32).to(DEV)


# -- quantiser ------------------------------------------------------------------
def _ties(n):
    """Up to n values, in units of the scale, that sit exactly between two
    e4m3fn codes: the subnormal midpoints (2m + 1) * 2^-10 (the first is
    2^-10, half the smallest code) and midpoints (1 + (2j + 1) / 16) * 2^e of
    the normal codes, odd and even mantissas below them; both signs.  Every
    one is exact in bf16 (four fraction bits)."""
    sub = [(2 * m + 1) * 2.0 ** -10 for m in range(8)]
    nor = [(1 + (2 * j + 1) / 16) * 2.0 ** e for e in (-6, -3, 0, 4, 7) for j in range(8)]
    vals = [s * t for t in sub + nor for s in (1.0, -1.0)]
    return torch.tensor(vals[:n])


def _kv_input(R, S, H, hd, dtype, seed):
    """(R, S, 2d): K and V side by side, as the K/V projection leaves them.
    Inside every head the magnitudes spread over 2^16, so subnormal codes
    occur; row 2 head 0 of K is zero; row 3 head 1 of K holds 448 * 2^-3 (so
    its scale is exactly 2^-3) and exact ties in units of that scale."""
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    x = torch.randn(R, S, 2 * d, generator=g) * 2.0 ** (torch.rand(R, S, 2 * d, generator=g) * -16)
    x *= 10.0 ** (torch.rand(R, 1, 2 * H, generator=g) * 6 - 3).repeat_interleave(hd, 2)
    x[2, :, :hd] = 0
    head = x[3, :, hd:2 * hd]
    flat = (head.reshape(-1) * 0.0)
    flat[0] = 448.0 * 2.0 ** -3
    t = _ties(flat.numel() - 1) * 2.0 ** -3
    flat[1:1 + t.numel()] = t
    x[3, :, hd:2 * hd] = flat.reshape(S, hd)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_quantiser_is_bit_identical_to_the_reference(H, hd, dtype):
    from mtts.attn_kernels import quantize_kv_fp8
    d = H * hd
    for S in (1, 5, _ck(hd) + 1):
        lens = [0, 1, S - 1, S, S + 3]                      # the last is clamped to S
        kv = _kv_input(5, S, H, hd, dtype, seed=S)
        kvd = kv.to(DEV)
        for name, view, cpu in (("k", kvd[..., :d], kv[..., :d]), ("v", kvd[..., d:], kv[..., d:])):
            for n in (lens, None):
                q8, scale = quantize_kv_fp8(view, H, _i32(n))
                assert q8.shape == (5, H, S, hd) and q8.dtype == torch.uint8 and q8.is_contiguous()
                assert scale.shape == (5, H) and scale.dtype == torch.float32
                want8, wscale = quantize_ref(cpu, H, None if n is None else torch.tensor(n))
                assert torch.equal(scale.cpu(), wscale), f"{name} scale, S={S}, lens={n}"
                bad = (q8.cpu() != want8).nonzero()
                assert bad.numel() == 0, f"{name} bytes, S={S}, lens={n}: first mismatch at {bad[0].tolist()}"
        # the planted cases are what they claim to be
        q8, scale = quantize_ref(kv[..., :d], H)
        assert scale[2, 0] == 1 and (q8[2, 0] == 0).all()
        assert scale[3, 1] == 2.0 ** -3 and q8[3, 1, 0, 0] == 0x7E
        if S * hd > 16:
            codes = q8[3, 1].flatten()[1:17]
            assert codes[0] == 0 and codes[1] == 0x80       # +-2^-10: a tie between 0 and the smallest code, to even
            assert ((codes & 0x7F) <= 8).all()              # the subnormal codes; 7.5 ties up to the first normal one


def test_quantiser_writes_one_slot_of_a_larger_buffer():
    from mtts.attn_kernels import quantize_kv_fp8
    H, hd, S = 2, 64, 261
    x = _kv_input(4, S, H, hd, torch.bfloat16, seed=3)[1:2, :, :H * hd].to(DEV)
    out = torch.full((3, H, S, hd), 0xAB, dtype=torch.uint8, device=DEV)
    sc = torch.full((3, H), 7.0, device=DEV)
    n = _i32([200])
    quantize_kv_fp8(x, H, n, out=out[1:2], scale_out=sc[1:2])
    want8, wscale = quantize_ref(x.cpu(), H, torch.tensor([200]))
    assert torch.equal(out[1:2].cpu(), want8) and torch.equal(sc[1:2].cpu(), wscale)
    assert (out[[0, 2]] == 0xAB).all() and (sc[[0, 2]] == 7.0).all()
    assert (out[1, :, 200:] == 0).all()


def test_quantiser_non_finite_gives_nan_scale():
    from mtts.attn_kernels import quantize_kv_fp8
    x = torch.randn(2, 9, 128, device=DEV)
    x[0, 3, 70] = float("inf")
    x[1, 8, 5] = float("nan")
    _, scale = quantize_kv_fp8(x, 2, _i32([9, 8]))
    assert torch.isnan(scale[0, 1]) and torch.isfinite(scale[0, 0])
    assert torch.isfinite(scale[1]).all()                   # the NaN sits past row 1's count


# -- attention -------------------------------------------------------------------
def _make(B, S, H, hd, dtype, seed, mask=True):
    """q (B, d) in `dtype`, quantised K / V of B rows over S keys (every key
    counted, so that a test may pick any count afterwards) and a mask."""
    from mtts.attn_kernels import quantize_kv_fp8
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = H * hd
    q = torch.randn(B, d, device=DEV, generator=g).to(dtype)
    kv = torch.randn(B, S, 2 * d, device=DEV, generator=g).to(torch.bfloat16)
    kpm = None
    if mask:
        kpm = torch.rand(B, S, device=DEV, generator=g) < 0.3
        kpm[:, 0] = False
    k8, ks = quantize_kv_fp8(kv[..., :d], H)
    v8, vs = quantize_kv_fp8(kv[..., d:], H)
    return q, k8, v8, ks, vs, kpm


def _fp8(q, k8, v8, ks, vs, H, kpm=None, lens=None, **kw):
    from mtts.attn_kernels import attention_decode_split_fp8
    return attention_decode_split_fp8(q, k8, v8, ks, vs, H, kpm, _i32(lens), **kw)


def _check_rows(out, lse, q, k8, v8, ks, vs, H, kpm, lens, dtype):
    """Every row against the float64 reference on the dequantised first lens[b] keys."""
    tol, ltol = (2e-5 if dtype == torch.float32 else 2e-2), 1e-5
    S = k8.shape[2]
    kh = to_channel_last(dequantize_ref(k8, ks)).to(DEV)
    vh = to_channel_last(dequantize_ref(v8, vs)).to(DEV)
    for b in range(q.shape[0]):
        n = S if lens is None else min(lens[b], S)
        m = None if kpm is None else kpm[b:b + 1, :n]
        ref, ref_lse = ref_attention(q[b:b + 1, None], kh[b:b + 1, :n], vh[b:b + 1, :n], H, m)
        close(out[b:b + 1, None], ref, tol)
        close(lse[b:b + 1, :, None], ref_lse, ltol)


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_parity_at_the_chunk_edges(H, hd, dtype, mask):
    ck = _ck(hd)
    for S in (5, ck, ck + 1, 2 * ck, 2 * ck + 3):
        q, k8, v8, ks, vs, kpm = _make(5, S, H, hd, dtype, seed=S % 97, mask=mask)
        lens = [1, ck, ck + 1, S, 7]                        # a count past S means S: the kernel clamps it
        out, lse = _fp8(q, k8, v8, ks, vs, H, kpm, lens, want_lse=True)
        assert out.shape == (5, H * hd) and out.dtype == dtype and lse.shape == (5, H)
        _check_rows(out, lse, q, k8, v8, ks, vs, H, kpm, lens, dtype)
    out, lse = _fp8(q, k8, v8, ks, vs, H, kpm, None, want_lse=True)
    _check_rows(out, lse, q, k8, v8, ks, vs, H, kpm, None, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_bytes_past_the_count_and_other_rows_scales_do_not_reach_the_result(H, hd, dtype):
    ck = _ck(hd)
    S = 2 * ck + 3
    q, k8, v8, ks, vs, kpm = _make(5, S, H, hd, dtype, seed=5)
    lens = [1, ck, ck + 1, S, 7]
    want, wlse = _fp8(q, k8, v8, ks, vs, H, kpm, lens, want_lse=True)
    k8, v8 = k8.clone(), v8.clone()
    for b, n in enumerate(lens):
        k8[b, :, n:] = 0x7F                                 # NaN in e4m3fn
        v8[b, :, n:] = 0x7F
    got, lse = _fp8(q, k8, v8, ks, vs, H, kpm, lens, want_lse=True)
    assert torch.equal(got, want) and torch.equal(lse, wlse)
    for b in (0, 2, 4):                                     # every other row's scales NaN
        ks2, vs2 = torch.full_like(ks, float("nan")), torch.full_like(vs, float("nan"))
        ks2[b], vs2[b] = ks[b], vs[b]
        got, lse = _fp8(q, k8, v8, ks2, vs2, H, kpm, lens, want_lse=True)
        assert torch.equal(got[b], want[b]) and torch.equal(lse[b], wlse[b])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,hd", SHAPES)
def test_a_row_is_the_same_bits_anywhere(H, hd, dtype):
    ck = _ck(hd)
    S = 2 * ck + 3
    q, k8, v8, ks, vs, kpm = _make(20, S, H, hd, dtype, seed=9)
    lens = [(7 * b * ck // 5) % S + 1 for b in range(20)]
    lens[3], lens[17] = ck + 1, S
    full, flse = _fp8(q, k8, v8, ks, vs, H, kpm, lens, want_lse=True)
    five, _ = _fp8(q[:5], k8[:5], v8[:5], ks[:5], vs[:5], H, kpm[:5], lens[:5], want_lse=True)
    assert torch.equal(five[3], full[3])
    for b in (3, 17):                                       # alone at batch 1
        one, olse = _fp8(q[b:b + 1], k8[b:b + 1], v8[b:b + 1], ks[b:b + 1], vs[b:b + 1], H, kpm[b:b + 1],
                         lens[b:b + 1], want_lse=True)
        assert torch.equal(one[0], full[b]) and torch.equal(olse[0], flse[b])
    # a workspace given or allocated
    from mtts.attn_kernels import decode_split_workspace
    ws = torch.empty(decode_split_workspace(20, H, hd, S) + 64, dtype=torch.uint8, device=DEV)
    again = _fp8(q, k8, v8, ks, vs, H, kpm, lens, workspace=ws)
    assert torch.equal(again, full)
    if dtype == torch.bfloat16:                             # the packed image holds the row-major bits
        yp = _fp8(q, k8, v8, ks, vs, H, kpm, lens, packed=True)
        assert torch.equal(yp.unpack()[:20], full)


@pytest.mark.parametrize("H,hd", SHAPES)
def test_empty_rows_and_a_fully_masked_middle_chunk(H, hd):
    ck = _ck(hd)
    S = 2 * ck + 3
    dtype = torch.float32
    q, k8, v8, ks, vs, kpm = _make(4, S, H, hd, dtype, seed=11)
    kpm[1] = True                                           # row 1: every key masked
    kpm[3, ck:2 * ck] = True                                # row 3: the middle chunk masked
    lens = [0, S, S, S]                                     # row 0: no key
    out, lse = _fp8(q, k8, v8, ks, vs, H, kpm, lens, want_lse=True)
    for b in (0, 1):
        assert torch.isnan(out[b]).all() and (lse[b] == float("-inf")).all()
    kh = to_channel_last(dequantize_ref(k8, ks)).to(DEV)
    vh = to_channel_last(dequantize_ref(v8, vs)).to(DEV)
    for b in (2, 3):                                        # the neighbours are untouched
        ref, ref_lse = ref_attention(q[b:b + 1, None], kh[b:b + 1], vh[b:b + 1], H, kpm[b:b + 1])
        close(out[b:b + 1, None], ref, 2e-5)
        close(lse[b:b + 1, :, None], ref_lse, 1e-5)
    alone, alse = _fp8(q[3:], k8[3:], v8[3:], ks[3:], vs[3:], H, kpm[3:], [S], want_lse=True)
    assert torch.equal(alone[0], out[3]) and torch.equal(alse[0], lse[3])
