"""The model half of a decode context: the decoder's constants cast once per
context, the packed images of its projection weights, and the decision which
step runs over them at a row count.  It holds the per-request half, the
Conditioning of mtts/conditioning.py, whose layers are added here."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from . import ops
from .attn_kernels import decode_split_chunk
from .linear import cast_weight


def _options():
    from .decode import DecodeEngine    # the routing switches stay on the engine: the A/B tools set them there
    return DecodeEngine.OPTIONS


class Projection:
    """A packable projection of the step: `w` the row-major weight, `ln`
    whether it runs with a LayerNorm prologue, `packed` its image in MFMA
    fragment order (csrc/gemv.hip), None until pack_weights makes it."""

    def __init__(self, w, ln=False):
        self.w, self.ln, self.packed = w, ln, None

    @property
    def operand(self):   # what the fused step hands to gemm_rows: the packed image when there is one
        return self.w if self.packed is None else self.packed


class Layer(SimpleNamespace):
    """Win, Wx, Wout, Wq, Wo, W1, W2 as Projections; Wdt, the biases bq / bo /
    b1 / b2 and the fp32 conv_w, conv_b, A, D, dt_bias as plain tensors."""

    def projections(self):
        return (self.Win, self.Wx, self.Wout, self.Wq, self.Wo, self.W1, self.W2)


def fused_ok(model, cd, rows, use_rows):
    """The fused-epilogue step (_step_rows) applies: bf16, <= 32 rows and
    the shapes csrc/rows.hip takes (checked once per context)."""
    m = model
    if not use_rows or cd != torch.bfloat16 or rows > ops.GEMM_ROWS_MAX or not _options()["fused"]:
        return False
    d = m.token_embed.weight.shape[1]
    if not ops.gemm_rows_ln_ok(d):
        return False
    for l in m.layers:
        mm = l.mamba
        if (mm.d_conv != 4 or d % 64 or mm.d_inner % 64 or d % 8 or d > 2048 or l.ff[0].weight.shape[0] % 64
                or any(n.weight.dtype != torch.float32 for n in (l.norm_mamba, l.norm_cross, l.norm_ff))):
            return False
    return m.norm_out.weight.dtype == torch.float32


class DecodeContext:
    """cond, cd, rows (cond's); layers (Layer records); tok_w / pos_w fp32,
    q0_w / q0_id the zero quantizer row of the embedding launch; the head Wh
    (a Projection) and bh; use_rows, the engine's; and the routing latch()
    decides, False until then: fused, xpk, fuse_q."""

    def __init__(self, model, cond, use_rows=True):
        """The context over `cond` (Conditioning.from_batch or .idle), whose layers are added here."""
        m = self.m = model
        cd = cond.cd
        d = m.token_embed.weight.shape[1]
        dev = m.token_embed.weight.device
        self.cond, self.cd, self.rows, self.use_rows, self.layers = cond, cd, cond.rows, use_rows, []
        self.fused = self.xpk = self.fuse_q = False
        for l in m.layers:
            ca = l.cross_attn
            W = cast_weight(ca.in_proj_weight, cd)
            b = cast_weight(ca.in_proj_bias, cd)
            cond.add_layer(l, W[d:], b[d:])
            mm = l.mamba
            di = mm.d_inner
            self.layers.append(Layer(
                Wq=Projection(W[:d], ln=True), bq=b[:d],
                Wo=Projection(cast_weight(ca.out_proj.weight, cd)), bo=cast_weight(ca.out_proj.bias, cd),
                W1=Projection(cast_weight(l.ff[0].weight, cd), ln=True), b1=cast_weight(l.ff[0].bias, cd),
                W2=Projection(cast_weight(l.ff[2].weight, cd)), b2=cast_weight(l.ff[2].bias, cd),
                Win=Projection(cast_weight(mm.in_proj.weight, cd), ln=True),
                Wx=Projection(cast_weight(mm.x_proj.weight, cd)),
                Wdt=cast_weight(mm.dt_proj.weight, cd), Wout=Projection(cast_weight(mm.out_proj.weight, cd)),
                conv_w=mm.conv1d.weight.detach().reshape(di, -1).float().contiguous(),
                conv_b=mm.conv1d.bias.detach().float().contiguous(),
                A=(-torch.exp(mm.A_log.detach().float())).contiguous(), D=mm.D.detach().float().contiguous(),
                dt_bias=mm.dt_proj.bias.detach().float().contiguous(),
            ))
        cond.source = None
        self.tok_w = m.token_embed.weight.detach().float().contiguous()
        self.pos_w = m.pos_embed.weight.detach().float().contiguous()
        self.q0_w = torch.zeros(1, d, device=dev)
        self.q0_id = torch.zeros(1, device=dev, dtype=torch.int32)
        self.Wh, self.bh = Projection(cast_weight(m.head.weight, cd), ln=True), cast_weight(m.head.bias, cd)

    @classmethod
    def build(cls, model, cond, rows, use_rows=True):
        """The context over `cond`, routed for `rows` rows: what an engine adopts."""
        ctx = cls(model, cond, use_rows)
        ctx.latch(rows)
        return ctx

    def projections(self):
        """Every packable projection, the layers' in step order, then the head."""
        return [p for l in self.layers for p in l.projections()] + [self.Wh]

    def pack_weights(self):
        """Packed (MFMA-fragment order) images of the step's projection
        weights for csrc/gemv.hip, made once per context; shapes the packed
        kernel does not take keep the row-major weight."""
        for p in self.projections():
            if ops.gemv_split_ok(p.w.shape[1], ln=p.ln):
                p.packed = ops.pack_rows_weight(p.w)

    def xpk_ok(self):
        """Every projection packed and every operand shape the packed
        activation images take (K, N % 32; a key side the single-pass or the
        split-key kernel takes): the step of _step_xpk applies; makes nothing."""
        if not _options()["xpacked"] or any(p.packed is None for p in self.projections()):
            return False
        for l, p in zip(self.m.layers, self.layers):
            ca = l.cross_attn
            hd = ca.embed_dim // ca.num_heads
            if (any(q.w.shape[0] % 32 or q.w.shape[1] % 32 for q in p.projections())
                    or (self.cond.keys > decode_split_chunk(hd) and not self.cond.splits(hd))
                    or l.mamba.d_inner % 32):
                return False
        return True

    def fuse_q_ok(self, rows):
        """Shapes mtts_attention_decode_qproj takes (head_dim 64 / 128,
        d_model <= 2048, <= 32 sequences, no FP8 keys, the single-pass range)."""
        cond = self.cond
        for l, p in zip(self.m.layers, self.layers):
            ca = l.cross_attn
            hd = ca.embed_dim // ca.num_heads
            if (cond.fp8 or hd not in (64, 128) or ca.embed_dim > 2048 or ca.embed_dim % 8 or rows > 32
                    or cond.keys > decode_split_chunk(hd) or p.Wq.w.stride(0) != ca.embed_dim):
                return False
        return True

    def latch(self, rows):
        """Which step runs over the context at `rows` rows, decided once per
        context: the fused-epilogue step, its packed weights, the packed
        activations (with the head-major K / V and the packed FiLM images
        they read) and the q projection inside the attention kernel.  The
        split-key routing was latched with `cond`: xpk_ok and every later
        step agree on it."""
        opt = _options()
        self.fused = fused_ok(self.m, self.cd, rows, self.use_rows)
        if self.fused and opt["packed"]:
            self.pack_weights()
        self.xpk = self.fused and self.xpk_ok()
        if self.xpk:
            self.cond.make_packed_images()
        self.fuse_q = self.xpk and opt["fuse_q"] and self.fuse_q_ok(rows)
