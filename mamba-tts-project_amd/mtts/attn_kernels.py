"""Multi-head attention core o = softmax(q k^T / sqrt(hd) + mask) v on the HIP
kernels of libmtts (mtts_attention_fwd / _bwd, csrc/attn.hip).

q (B, T, H*hd), k/v (B, S, H*hd) channel-last (head-major inside the row, as
nn.MultiheadAttention's projections produce; reference call sites
mamba_decoder.py:72-77, style_cross_attention.py:125-131,270-276).
key_padding_mask (B, S) bool, True = ignore.  Fully masked rows produce NaN
(PyTorch MHA semantics).

Attention-weight dropout (only the style pipeline's training mode uses it,
style_cross_attention.py:91-96) has no HIP kernel: that case runs torch's
scaled_dot_product_attention, whose RNG stream no reimplementation could
match anyway.  Everything else runs on libmtts, and there is no CPU path.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib as L

_HEAD_DIMS = (16, 32, 64, 128)


def _aligned(t):
    es = t.element_size()
    return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and (t.stride(0) * es) % 16 == 0
            and (t.stride(1) * es) % 16 == 0)


def _prep(t):
    return t if _aligned(t) else t.contiguous()


def _fwd_args(q, k, v, n_heads, kpm, out, lse):
    B, T, d = q.shape
    a = L.AttnFwdArgs()
    a.batch, a.heads, a.head_dim, a.q_len, a.kv_len = B, n_heads, d // n_heads, T, k.shape[1]
    a.dtype = L.dtype_code(q)
    a.scale = 1.0 / math.sqrt(d // n_heads)
    a.q_bs, a.q_ls = q.stride(0), q.stride(1)
    a.k_bs, a.k_ls = k.stride(0), k.stride(1)
    a.v_bs, a.v_ls = v.stride(0), v.stride(1)
    a.o_bs, a.o_ls = out.stride(0), out.stride(1)
    a.mask_bs = 0 if kpm is None else kpm.stride(0)
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.key_padding_mask = L.ptr(kpm)
    a.out = out.data_ptr()
    a.lse = L.ptr(lse)
    return a


def _mask_u8(kpm, B, S):
    if kpm is None:
        return None
    if kpm.shape != (B, S):
        raise ValueError(f"key_padding_mask must be (B, S) = {(B, S)}, got {tuple(kpm.shape)}")
    if kpm.dtype != torch.bool:
        raise TypeError("key_padding_mask must be bool (True = ignore)")
    kpm = kpm.contiguous()
    return kpm.view(torch.uint8)


def _decode_args(who, q, k, v, n_heads, kpm, want_out, want_packed, kv_batch=None):
    """The front end of the single-query calls: AttnFwdArgs for q (B, d)
    against k / v (B, S, d) channel-last or HEAD-MAJOR (B, H, S, hd)
    contiguous (one contiguous K and V block per (batch, head): kv_hs), the
    mask as bytes, and the outputs asked for.  Returns (args, out (B, 1, d) or
    None, PackedAct or None, keep); `keep` holds the aligned copies the
    pointers in args may refer to and must live until the launch.  `who`
    names the caller in the errors.  kv_batch: the rows of k / v / kpm when
    they are not q's (the shared-key call)."""
    from .ops import PackedAct
    B, d = q.shape
    R = B if kv_batch is None else kv_batch
    if k.shape[0] != R or v.shape[0] != R:
        raise ValueError(f"{who}: k / v must have {R} rows")
    q3 = q[:, None]
    if not _aligned(q3):
        q3 = q3.contiguous()
    out = torch.empty(B, 1, d, device=q.device, dtype=q.dtype) if want_out else None
    yp = PackedAct.empty(B, d, q.device) if want_packed else None
    o3 = q3 if out is None else out                         # strides only: no row-major out
    if k.dim() == 4:
        H, S, hd = k.shape[1:]
        if H != n_heads or H * hd != d or k.shape != v.shape or not (k.is_contiguous() and v.is_contiguous()):
            raise ValueError(f"{who}: head-major k / v must be contiguous (B, H, S, hd)")
        m = _mask_u8(kpm, R, S)
        a = _fwd_args(q3, k.view(R, H * S, hd), v.view(R, H * S, hd), n_heads, m, o3, None)
        a.kv_len, a.k_ls, a.v_ls, a.kv_hs = S, hd, hd, S * hd
    else:
        k, v = _prep(k), _prep(v)
        m = _mask_u8(kpm, R, k.shape[1])
        a = _fwd_args(q3, k, v, n_heads, m, o3, None)
    a.out = 0 if out is None else out.data_ptr()
    a.out_packed = None if yp is None else yp.data.data_ptr()
    return a, out, yp, (q3, k, v, m)


def attention_decode_packed(q, k, v, n_heads, kpm=None):
    """Single-query attention (q (B, d), decode step) returning the output
    as the packed activation image of the output projection (ops.PackedAct;
    csrc/attn.hip single-pass decode kernel).  k / v: (B, S, d) channel-last,
    or HEAD-MAJOR (B, H, S, hd) contiguous (the decode engine's per-context
    copies): one contiguous K and V block per (batch, head)."""
    # the row-major out is allocated and stored as well (as it always was: the captured graphs hold that store)
    a, out, yp, keep = _decode_args("attention_decode_packed", q, k, v, n_heads, kpm, want_out=True, want_packed=True)
    L.call("mtts_attention_fwd", a)
    return yp


def attention_decode_qproj_packed(x, wq, bq, ln_w, ln_b, eps, k, v, n_heads, kpm=None):
    """Single-query cross-attention with the query projection fused in
    (mtts_attention_decode_qproj): q = bf16(LN(x) wq^T + bq) per (batch,
    head) inside the decode kernel, LN(x) = bf16(LayerNorm(x) * ln_w + ln_b)
    as the packed projections' LayerNorm prologue computes it; k / v
    head-major (B, H, S, hd) contiguous.  Returns the output as the packed
    activation image of the output projection (ops.PackedAct)."""
    B, d = x.shape
    if k.dim() != 4 or not (k.is_contiguous() and v.is_contiguous()):
        raise ValueError("attention_decode_qproj_packed: head-major contiguous (B, H, S, hd) k / v")
    if x.dtype != torch.bfloat16 or x.stride(1) != 1 or wq.dtype != torch.bfloat16 or wq.stride(1) != 1 \
            or wq.stride(0) != d:
        raise ValueError("attention_decode_qproj_packed: bf16 x (B, d) and row-major bf16 wq (d, d)")
    # x stands in for q (the kernel computes q; the C side checks x itself): no row-major out
    a, _, yp, keep = _decode_args("attention_decode_qproj_packed", x, k, v, n_heads, kpm, want_out=False,
                                  want_packed=True)
    qa = L.AttnQProjArgs()
    qa.f = a
    qa.x, qa.x_rs = x.data_ptr(), x.stride(0)
    qa.wq, qa.bq = wq.data_ptr(), L.ptr(bq)
    lw, lb = ln_w.detach().float().contiguous(), ln_b.detach().float().contiguous()
    qa.ln_w, qa.ln_b, qa.eps, qa.d_model = lw.data_ptr(), lb.data_ptr(), float(eps), d
    L.call("mtts_attention_decode_qproj", qa)
    return yp


def decode_split_chunk(hd):
    """Keys per workgroup of the split-key single-query kernel: what the
    single-pass decode kernel holds in registers, a function of the head dim
    alone (csrc/attn.hip attn_decode_split_kernel)."""
    if hd not in _HEAD_DIMS:
        raise ValueError(f"head_dim {hd} not supported (need one of {_HEAD_DIMS})")
    return 16384 // hd


def key_counts(keep):
    """A row's key count: the index of its last kept key + 1, 0 for a row
    that keeps none.  keep (B, S) bool, True = attend; returns (B,) int32 on
    keep's device, without a host synchronisation.  Keys below the count may
    still be masked (the padding of a reference prompt inside [ref ‖ text]);
    keys at or past it are never read by attention_decode_split."""
    if keep.dim() != 2 or keep.dtype != torch.bool:
        raise TypeError("key_counts: keep must be (B, S) bool (True = attend)")
    B, S = keep.shape
    if S == 0:
        return torch.zeros(B, dtype=torch.int32, device=keep.device)
    idx = torch.arange(1, S + 1, dtype=torch.int32, device=keep.device)
    return (keep.to(torch.int32) * idx).amax(dim=1)


def decode_split_workspace(B, n_heads, hd, S):
    """Bytes of fp32 partials attention_decode_split needs (at least 4, so
    that an empty batch still has an address to pass)."""
    return max(int(L.lib().mtts_attention_decode_split_workspace(B, n_heads, hd, S)), 4)


def attention_decode_split(q, k, v, n_heads, kpm=None, kv_lens=None, packed=False, want_lse=False, workspace=None,
                           kv_rows=None):
    """Single-query attention over a long key side (mtts_attention_decode_split:
    one workgroup per (batch, head, chunk of decode_split_chunk(hd) keys), then
    a merge in chunk order).  q (B, d); k / v (B, S, d) channel-last or
    head-major (B, H, S, hd) contiguous; kpm (B, S) bool, True = ignore;
    kv_lens (B,) int32 on the device: row b attends to its first kv_lens[b]
    keys only and reads no other.  Returns the (B, d) output, or its packed
    activation image (ops.PackedAct; bf16, B <= 32) when `packed`; with
    want_lse also the (B, H) fp32 log-sum-exp.  workspace: a uint8 device
    tensor of decode_split_workspace(B, H, hd, S) bytes to keep the partials
    in (the decode engine holds one per context); None allocates one.
    kv_rows (B,) int32 on the device (mtts_attention_decode_split_shared):
    k / v / kpm / kv_lens then have R rows of their own, query row b reads
    K/V row kv_rows[b] with that row's mask and count, and rows with equal
    values share one load of every chunk; each row's result is the bits the
    call without kv_rows gives on k[kv_rows], v[kv_rows], ...  A value
    outside [0, R) gives the row no keys (NaN, lse -inf).  None: today's
    symbol, k / v per query row."""
    who = "attention_decode_split"
    B = _split_rows(who, q, n_heads, k, v)
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("q, k, v must share a dtype")
    R = B
    if kv_rows is not None:
        if kv_rows.dtype != torch.int32 or tuple(kv_rows.shape) != (B,) or not kv_rows.is_cuda \
                or not kv_rows.is_contiguous():
            raise ValueError(f"attention_decode_split: kv_rows must be ({B},) int32 on the device")
        R = k.shape[0]
        if R < 1:
            raise ValueError("attention_decode_split: kv_rows needs at least one K/V row")
    sa, res, keep = _split_args(who, q, k, v, n_heads, kpm, kv_lens, packed, want_lse, workspace, R)
    if kv_rows is None:
        L.call("mtts_attention_decode_split", sa)
    else:
        sh = L.AttnDecodeSplitSharedArgs()
        sh.s, sh.kv_rows, sh.kv_batch = sa, kv_rows.data_ptr(), R
        L.call("mtts_attention_decode_split_shared", sh)
    return res


def _split_rows(who, q, n_heads, *operands):
    """What a split-key call checks first, under the caller's name `who`; returns q's rows."""
    for t in (q,) + operands:
        if not t.is_cuda:
            raise RuntimeError("libmtts ops need CUDA (HIP) tensors; there is no CPU path")
    if q.dim() != 2:
        raise ValueError(f"{who}: q must be (B, d)")
    B, d = q.shape
    if d % n_heads or (d // n_heads) not in _HEAD_DIMS:
        raise ValueError(f"head_dim {d}/{n_heads} not supported (need one of {_HEAD_DIMS})")
    return B


def _split_args(who, q, k, v, n_heads, kpm, kv_lens, packed, want_lse, workspace, R):
    """What a split-key call checks after its own checks, in this order: the single-query front end over R rows
    of k / v, the key side, kv_lens, the workspace.  Returns AttnDecodeSplitArgs, what the caller returns after
    its launch, and the tensors that must live until then."""
    B = q.shape[0]
    a, out, yp, keep = _decode_args(who, q, k, v, n_heads, kpm, want_out=not packed, want_packed=packed, kv_batch=R)
    if a.kv_len < 1:
        raise ValueError(f"{who}: the key side is empty")
    lse = torch.empty(B, n_heads, device=q.device, dtype=torch.float32) if want_lse else None
    a.lse = L.ptr(lse)
    _check_kv_lens(who, kv_lens, R)
    sa = L.AttnDecodeSplitArgs()
    sa.f, sa.kv_lens = a, L.ptr(kv_lens)
    nbytes = decode_split_workspace(B, n_heads, q.shape[1] // n_heads, a.kv_len)
    ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8) if workspace is None else workspace
    if ws.dtype != torch.uint8 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < nbytes:
        raise ValueError(f"{who}: workspace must be >= {nbytes} contiguous uint8 bytes on the device")
    sa.workspace, sa.workspace_bytes = ws.data_ptr(), ws.numel()
    res = yp if packed else out[:, 0]
    return sa, ((res, lse) if want_lse else res), (keep, ws)


def _check_kv_lens(who, kv_lens, R):
    if kv_lens is not None and (kv_lens.dtype != torch.int32 or tuple(kv_lens.shape) != (R,) or not kv_lens.is_cuda
                                or not kv_lens.is_contiguous()):
        raise ValueError(f"{who}: kv_lens must be ({R},) int32 on the device")


def quantize_kv_fp8(x, n_heads, kv_lens=None, out=None, scale_out=None):
    """K or V of a conditioning sequence as OCP FP8 (e4m3fn) with one fp32
    scale per (row, head) (mtts_kv_quantize_fp8, csrc/kvq.hip).  x (R, S, d)
    bf16 / fp32 channel-last with unit inner stride -- a column view of the
    (R, S, 2d) K/V projection is taken as it is; kv_lens (R,) int32 on the
    device: row r's first kv_lens[r] keys (clamped to [0, S]) count, None: S.
    Returns (bytes (R, H, S, hd) torch.uint8, head-major, scale (R, H) fp32):
    scale = max |x| over the head's counted keys / 448 (1 for an all-zero
    head), bytes = (x.float() / scale).to(torch.float8_e4m3fn) bit for bit for
    the counted keys and 0 for the others.  A NaN or infinity among a head's
    counted keys makes its scale NaN.  out / scale_out: where to write, e.g.
    one slot's rows of a session's buffers (out[r] contiguous, scale_out[r]
    contiguous; the rows may be strided); other rows are not touched."""
    if not x.is_cuda:
        raise RuntimeError("libmtts ops need CUDA (HIP) tensors; there is no CPU path")
    if x.dim() != 3:
        raise ValueError("quantize_kv_fp8: x must be (R, S, d)")
    R, S, d = x.shape
    if d % n_heads or (d // n_heads) not in _HEAD_DIMS:
        raise ValueError(f"head_dim {d}/{n_heads} not supported (need one of {_HEAD_DIMS})")
    hd = d // n_heads
    _check_kv_lens("quantize_kv_fp8", kv_lens, R)
    x = _prep(x)
    if out is None:
        out = torch.empty(R, n_heads, S, hd, device=x.device, dtype=torch.uint8)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != (R, n_heads, S, hd) or not out.is_cuda
          or (R and not out[0].is_contiguous())):
        raise ValueError(f"quantize_kv_fp8: out must be ({R}, {n_heads}, {S}, {hd}) uint8 on the device, rows contiguous")
    if scale_out is None:
        scale_out = torch.empty(R, n_heads, device=x.device, dtype=torch.float32)
    elif (scale_out.dtype != torch.float32 or tuple(scale_out.shape) != (R, n_heads) or not scale_out.is_cuda
          or scale_out.stride(1) != 1):
        raise ValueError(f"quantize_kv_fp8: scale_out must be ({R}, {n_heads}) fp32 on the device, rows contiguous")
    a = L.KvQuantizeFp8Args()
    a.rows, a.heads, a.head_dim, a.kv_len, a.dtype = R, n_heads, hd, S, L.dtype_code(x)
    a.x_bs, a.x_ls = x.stride(0), x.stride(1)
    a.out_bs = out.stride(0) if R > 1 else n_heads * S * hd
    a.scale_bs = scale_out.stride(0) if R > 1 else n_heads
    a.x, a.kv_lens, a.out, a.scale = x.data_ptr(), L.ptr(kv_lens), out.data_ptr(), scale_out.data_ptr()
    nbytes = max(int(L.lib().mtts_kv_quantize_fp8_workspace(R, n_heads, hd, S)), 4)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.call("mtts_kv_quantize_fp8", a)
    return out, scale_out


def attention_decode_split_fp8(q, k8, v8, k_scale, v_scale, n_heads, kpm=None, kv_lens=None, packed=False,
                               want_lse=False, workspace=None):
    """attention_decode_split over FP8 K / V (mtts_attention_decode_split_fp8):
    k8 / v8 (B, H, S, hd) torch.uint8 head-major contiguous and k_scale /
    v_scale (B, H) fp32, as quantize_kv_fp8 returns them; q (B, d) bf16 or
    fp32, the dtype of the output.  With K^ = deq(k8) * k_scale and V^ alike,
    the result is softmax(q K^T / sqrt(hd)) V^ with fp32 accumulation; kpm,
    kv_lens, packed, want_lse and workspace (decode_split_workspace bytes) as
    attention_decode_split.  No byte at or past a row's count is read."""
    who = "attention_decode_split_fp8"
    B = _split_rows(who, q, n_heads, k8, v8, k_scale, v_scale)
    if k8.dtype != torch.uint8 or v8.dtype != torch.uint8 or k8.dim() != 4:
        raise TypeError("attention_decode_split_fp8: k8 / v8 must be (B, H, S, hd) torch.uint8 (e4m3fn bytes)")
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s.dtype != torch.float32 or tuple(s.shape) != (B, n_heads) or not s.is_contiguous():
            raise ValueError(f"attention_decode_split_fp8: {name} must be ({B}, {n_heads}) fp32, contiguous")
    fa = L.AttnDecodeSplitFp8Args()
    fa.s, res, keep = _split_args(who, q, k8, v8, n_heads, kpm, kv_lens, packed, want_lse, workspace, B)
    fa.k_scale, fa.v_scale, fa.scale_bs = k_scale.data_ptr(), v_scale.data_ptr(), n_heads
    L.call("mtts_attention_decode_split_fp8", fa)
    return res


def attention_fwd(q, k, v, n_heads, kpm=None, want_lse=False):
    """Returns (out (B, T, d) in q's dtype, lse (B, H, T) fp32 or None)."""
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError("libmtts ops need CUDA (HIP) tensors; there is no CPU path")
    B, T, d = q.shape
    if d % n_heads or (d // n_heads) not in _HEAD_DIMS:
        raise ValueError(f"head_dim {d}/{n_heads} not supported (need one of {_HEAD_DIMS})")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("q, k, v must share a dtype")
    q, k, v = _prep(q), _prep(k), _prep(v)
    m = _mask_u8(kpm, B, k.shape[1])
    out = torch.empty(B, T, d, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, n_heads, T, device=q.device, dtype=torch.float32) if want_lse else None
    L.call("mtts_attention_fwd", _fwd_args(q, k, v, n_heads, m, out, lse))
    return out, lse


def attention_bwd(q, k, v, n_heads, kpm, out, lse, dout, dk=None, dv=None, dq=None):
    """Returns (dq, dk, dv); dq/dk/dv may be given as (strided) output views."""
    B, T, d = q.shape
    S = k.shape[1]
    dout = _prep(dout.to(q.dtype))
    m = _mask_u8(kpm, B, S)
    if dq is None:
        dq = torch.empty_like(q, memory_format=torch.contiguous_format)
    if dk is None:
        dk = torch.empty(B, S, d, device=q.device, dtype=q.dtype)
    if dv is None:
        dv = torch.empty(B, S, d, device=q.device, dtype=q.dtype)
    a = L.AttnBwdArgs()
    a.f = _fwd_args(q, k, v, n_heads, m, out, lse)
    a.dout, a.do_bs, a.do_ls = dout.data_ptr(), dout.stride(0), dout.stride(1)
    a.dq, a.dq_bs, a.dq_ls = dq.data_ptr(), dq.stride(0), dq.stride(1)
    a.dk, a.dk_bs, a.dk_ls = dk.data_ptr(), dk.stride(0), dk.stride(1)
    a.dv, a.dv_bs, a.dv_ls = dv.data_ptr(), dv.stride(0), dv.stride(1)
    ws_bytes = L.lib().mtts_attention_bwd_workspace(B, n_heads, d // n_heads, T, S, L.dtype_code(q))
    ws = torch.empty(ws_bytes, device=q.device, dtype=torch.uint8)
    a.workspace = ws.data_ptr()
    L.call("mtts_attention_bwd", a)
    return dq, dk, dv


class AttentionFn(torch.autograd.Function):
    """Separate k / v inputs."""

    @staticmethod
    def forward(ctx, q, k, v, n_heads, kpm):
        q, k, v = _prep(q), _prep(k), _prep(v)
        out, lse = attention_fwd(q, k, v, n_heads, kpm, want_lse=True)
        ctx.save_for_backward(q, k, v, out, lse, kpm)
        ctx.n_heads = n_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, kpm = ctx.saved_tensors
        dq, dk, dv = attention_bwd(q, k, v, ctx.n_heads, kpm, out, lse, dout)
        return dq, dk, dv, None, None


class AttentionKVFn(torch.autograd.Function):
    """k = kv[..., :d], v = kv[..., d:] of one projection output: the gradient
    is written straight into one (B, S, 2d) tensor (no slice-backward copies)."""

    @staticmethod
    def forward(ctx, q, kv, n_heads, kpm):
        d = q.shape[-1]
        q = _prep(q)
        # the K/V gradient's destination when kv is a column view of the
        # layers' batched K/V projection (attention.KVAllFn / DkvSink)
        ctx.sink = getattr(kv, "_mtts_dkv_sink", None)
        if not _aligned(kv[..., :d]) or not _aligned(kv[..., d:]):
            kv = kv.contiguous()
        out, lse = attention_fwd(q, kv[..., :d], kv[..., d:], n_heads, kpm, want_lse=True)
        ctx.save_for_backward(q, kv, out, lse, kpm)
        ctx.n_heads = n_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, out, lse, kpm = ctx.saved_tensors
        d = q.shape[-1]
        dkv = None
        if ctx.sink is not None:
            sink, layer = ctx.sink
            dkv = sink.view(layer)
            if dkv.shape != kv.shape or not (_aligned(dkv[..., :d]) and _aligned(dkv[..., d:])):
                dkv = None
        if dkv is None:
            dkv = torch.empty(kv.shape, device=kv.device, dtype=kv.dtype)
        dq, _, _ = attention_bwd(q, kv[..., :d], kv[..., d:], ctx.n_heads, kpm, out, lse, dout,
                                 dk=dkv[..., :d], dv=dkv[..., d:])
        return dq, dkv, None, None


class AttentionQKVFn(torch.autograd.Function):
    """Self-attention on one fused projection output qkv (B, T, 3d): q, k, v
    are its thirds and the gradient is written straight into one (B, T, 3d)
    tensor (no slice-backward copies or adds)."""

    @staticmethod
    def forward(ctx, qkv, n_heads, kpm):
        d = qkv.shape[-1] // 3
        if not all(_aligned(qkv[..., i * d:(i + 1) * d]) for i in range(3)):
            qkv = qkv.contiguous()
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        out, lse = attention_fwd(q, k, v, n_heads, kpm, want_lse=True)
        ctx.save_for_backward(qkv, out, lse, kpm)
        ctx.n_heads = n_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, kpm = ctx.saved_tensors
        d = qkv.shape[-1] // 3
        dqkv = torch.empty(qkv.shape, device=qkv.device, dtype=qkv.dtype)
        attention_bwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], ctx.n_heads, kpm, out, lse, dout,
                      dq=dqkv[..., :d], dk=dqkv[..., d:2 * d], dv=dqkv[..., 2 * d:])
        return dqkv, None, None


def attention_qkv(qkv, n_heads, key_padding_mask=None, dropout_p=0.0):
    """Self-attention of q, k, v = the thirds of qkv (B, T, 3d)."""
    d = qkv.shape[-1] // 3
    if dropout_p > 0.0:
        return _sdpa_dropout(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], n_heads, key_padding_mask, dropout_p)
    if torch.is_grad_enabled() and qkv.requires_grad:
        return AttentionQKVFn.apply(qkv, n_heads, key_padding_mask)
    return attention_fwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], n_heads, key_padding_mask)[0]


def _sdpa_dropout(q, k, v, n_heads, key_padding_mask, dropout_p):
    B, T, d = q.shape
    S = k.shape[1]
    hd = d // n_heads
    qh = q.view(B, T, n_heads, hd).transpose(1, 2)
    kh = k.reshape(B, S, n_heads, hd).transpose(1, 2)
    vh = v.reshape(B, S, n_heads, hd).transpose(1, 2)
    mask = None
    if key_padding_mask is not None:
        mask = torch.zeros(B, 1, 1, S, device=q.device, dtype=q.dtype)
        mask = mask.masked_fill(key_padding_mask[:, None, None, :], float("-inf"))
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, dropout_p=dropout_p)
    return o.transpose(1, 2).reshape(B, T, d)


def attention(q, k, v, n_heads, key_padding_mask=None, dropout_p=0.0):
    if dropout_p > 0.0:
        return _sdpa_dropout(q, k, v, n_heads, key_padding_mask, dropout_p)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return AttentionFn.apply(q, k, v, n_heads, key_padding_mask)
    return attention_fwd(q, k, v, n_heads, key_padding_mask)[0]


def attention_kv(q, kv, n_heads, key_padding_mask=None, dropout_p=0.0):
    d = q.shape[-1]
    if dropout_p > 0.0:
        return _sdpa_dropout(q, kv[..., :d], kv[..., d:], n_heads, key_padding_mask, dropout_p)
    if torch.is_grad_enabled() and (q.requires_grad or kv.requires_grad):
        return AttentionKVFn.apply(q, kv, n_heads, key_padding_mask)
    return attention_fwd(q, kv[..., :d], kv[..., d:], n_heads, key_padding_mask)[0]
