"""The per-request half of a decode context: what the step reads of the
conditioning [ref ‖ text] and the style vector, one row per sequence of
generate() or slot of a session, and every operation on those rows."""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import ops
from .attn_kernels import (attention, attention_decode_packed, attention_decode_split, attention_decode_split_fp8,
                           decode_split_chunk, decode_split_workspace, key_counts, quantize_kv_fp8)

KV_IMAGES = ("k", "v", "khm", "vhm", "k8", "v8", "k_scale", "v_scale")


class Conditioning:
    """kpm (rows, keys) bool, True = ignore (None: no mask); kv_lens (rows,)
    int32 key counts; kv_rows (rows,) int32 in a share_keys session (query row
    r reads K/V row kv_rows[r]), else None; `split`, the split-key routing
    latched with the context, and split_ws, its workspace.  Per layer
    (`layers`) a record of H, Wkv / bkv (in_proj's K/V rows, cast), film (the
    style nn.Linear) and the images, None where one does not exist: k / v
    (column views of one (rows, keys, 2d) projection), khm / vhm / gamma_p /
    beta_p of a packed step, or -- "fp8" -- k8 / v8 e4m3fn bytes (rows, H,
    keys, hd) with k_scale / v_scale (rows, H) and no bf16 image.  DecodeContext
    (mtts/context.py) adds the layers beside the model's constants: one cast order."""

    def __init__(self, rows, keys, cd, kv_dtype, split, kpm, kv_lens, kv_rows=None, source=None):
        self.rows, self.keys, self.cd, self.fp8, self.split = rows, keys, cd, kv_dtype == "fp8", bool(split)
        self.kpm, self.kv_lens, self.kv_rows, self.split_ws = kpm, kv_lens, kv_rows, None
        self.layers, self.source = [], source               # source: from_batch's (th, z_style) while the layers go in

    @classmethod
    def from_batch(cls, model, text_hidden, z_style, text_mask, ref_hidden, ref_mask, cd, kv_dtype, split):
        """The rows of a conditioning batch (generate(), decode_step), projected as the layers are added."""
        th = text_hidden.to(cd)
        th, tm = model._concat_ref(th, text_mask, ref_hidden, ref_mask, th.shape[0], th.device)
        kpm = None if tm is None else ~tm                                   # mamba_decoder.py:68-70
        kv_lens = None if kpm is None else key_counts(~kpm)
        return cls(th.shape[0], th.shape[1], cd, kv_dtype, split, kpm, kv_lens, source=(th, z_style))

    @classmethod
    def idle(cls, rows, keys, cd, dev, kv_dtype, split, shared=False):
        """A session's idle rows, allocated as such: K / V zero (FP8: zero bytes,
        scale 1), FiLM rows zero, the mask ignoring every key but key 0 (a fully
        masked row would give NaN), count 1, kv_rows (`shared`) the identity."""
        kpm = torch.ones(rows, keys, dtype=torch.bool, device=dev)
        kpm[:, 0] = False
        return cls(rows, keys, cd, kv_dtype, split, kpm, torch.ones(rows, dtype=torch.int32, device=dev),
                   torch.arange(rows, dtype=torch.int32, device=dev) if shared else None)

    def add_layer(self, l, Wkv, bkv):
        """The next layer's rows, projected from `source` or idle.  Wkv (2d, d), bkv (2d,)."""
        B, S, d, dev, H = self.rows, self.keys, Wkv.shape[1], Wkv.device, l.cross_attn.num_heads
        c = SimpleNamespace(**dict.fromkeys(KV_IMAGES + ("gamma_p", "beta_p")), H=H, Wkv=Wkv, bkv=bkv, film=l.style_mlp[0])
        if self.source is None:
            if self.fp8:
                c.k8, c.v8 = (torch.zeros(B, H, S, d // H, device=dev, dtype=torch.uint8) for _ in range(2))
                c.k_scale, c.v_scale = torch.ones(B, H, device=dev), torch.ones(B, H, device=dev)
            else:
                kv = torch.zeros(B, S, 2 * d, device=dev, dtype=self.cd)
            c.gamma, c.beta = (torch.zeros(B, d, device=dev, dtype=self.cd) for _ in range(2))
        else:
            kv = self.project_kv(c, self.source[0]).view(B, -1, 2 * d)
            if self.fp8:
                c.k8, c.k_scale = quantize_kv_fp8(kv[..., :d], H, self.kv_lens)
                c.v8, c.v_scale = quantize_kv_fp8(kv[..., d:], H, self.kv_lens)
            gb = self.project_film(c, self.source[1])
            c.gamma, c.beta = gb[:, :d].contiguous(), gb[:, d:].contiguous()
        if not self.fp8:
            c.k, c.v = kv[..., :d], kv[..., d:]
        self.layers.append(c)

    @staticmethod                                           # generate() and a session's admission run these very GEMMs
    def project_kv(c, th):                                  # th (B, S, d) in the compute dtype -> K ‖ V (B * S, 2d)
        return torch.addmm(c.bkv, th.reshape(-1, c.Wkv.shape[1]), c.Wkv.t())

    def project_film(self, c, z):                           # z (B, d_style) -> gamma ‖ beta (B, 2d), compute dtype
        return torch.tanh(F.linear(z.to(c.film.weight.dtype), c.film.weight, c.film.bias)).to(self.cd)

    def splits(self, hd):
        """The key side goes to the split-key kernel: past the single-pass range, with OPTIONS["split_keys"] on at
        the build.  A head dim no attention kernel takes is not this predicate's to refuse: the call raises."""
        return self.split and hd in (16, 32, 64, 128) and self.keys > decode_split_chunk(hd)

    def make_packed_images(self):
        """What the packed step reads, made once it is chosen: head-major K / V (FP8 keys are) and packed FiLM rows."""
        for c in self.layers:
            if not self.fp8:
                B, S, d = c.k.shape
                c.khm = c.k.reshape(B, S, c.H, d // c.H).permute(0, 2, 1, 3).contiguous()
                c.vhm = c.v.reshape(B, S, c.H, d // c.H).permute(0, 2, 1, 3).contiguous()
        for c in self.layers:
            c.gamma_p, c.beta_p = ops.PackedAct.pack(c.gamma), ops.PackedAct.pack(c.beta)

    def attend(self, c, q, packed):
        """Every step's cross-attention of q (rows, d) over the layer's rows c, and the one place that picks its
        kernel.  FP8 keys (generate() / open_session saw to it that `splits` holds) or a long key side: the
        split-key kernel, its fp8 form for the former, with the key counts, kv_rows (rows with one value share
        one K/V row) and the workspace, one per context (every layer's partials have the same shape, the layers
        run in turn on one stream).  Else a packed step, which reads the head-major K / V, takes the
        single-pass kernel's packed image, a row-major step mtts_attention_fwd."""
        k, v = (c.k8, c.v8) if self.fp8 else (c.khm, c.vhm) if packed else (c.k, c.v)
        hd = q.shape[1] // c.H
        if self.fp8 or self.splits(hd):
            need = decode_split_workspace(q.shape[0], c.H, hd, self.keys)
            if self.split_ws is None or self.split_ws.numel() < need:
                self.split_ws = torch.empty(need, device=q.device, dtype=torch.uint8)
            if self.fp8:
                return attention_decode_split_fp8(q, k, v, c.k_scale, c.v_scale, c.H, self.kpm, self.kv_lens,
                                                  packed=packed, workspace=self.split_ws)
            return attention_decode_split(q, k, v, c.H, self.kpm, self.kv_lens, packed=packed,
                                          workspace=self.split_ws, kv_rows=self.kv_rows)
        if packed:
            return attention_decode_packed(q, k, v, c.H, self.kpm)
        return attention(q[:, None], k, v, c.H, self.kpm)[:, 0]

    def kv_bytes(self):
        """Bytes of every layer's K/V images (bf16: k, v and the head-major copies; fp8: bytes and scales)."""
        held = (getattr(c, name) for c in self.layers for name in KV_IMAGES)
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    def _put(self, c, r, k, v, gamma, beta, counts=None, src=None, keys=True):
        """Row r of c's images from k, v (keys, d) and gamma, beta (d,); `keys` false leaves K / V alone.  FP8
        keys are quantised into the row's bytes over counts ((1,) int32 on the device; the bytes past it zero);
        counts None: idle, zero bytes and scale 1; src: the row written from these very k, v, counts is copied."""
        if keys and not self.fp8:
            c.k[r].copy_(k)
            c.v[r].copy_(v)
            if c.khm is not None:
                c.khm[r].copy_(k.reshape(-1, c.H, k.shape[1] // c.H).permute(1, 0, 2))
                c.vhm[r].copy_(v.reshape(-1, c.H, k.shape[1] // c.H).permute(1, 0, 2))
        elif keys and src is not None:
            for t in (c.k8, c.v8, c.k_scale, c.v_scale):
                t[r].copy_(t[src])
        elif keys and counts is None:
            for t, idle in ((c.k8, 0), (c.v8, 0), (c.k_scale, 1.0), (c.v_scale, 1.0)):
                t[r].fill_(idle)
        elif keys:
            quantize_kv_fp8(k[None], c.H, counts, out=c.k8[r:r + 1], scale_out=c.k_scale[r:r + 1])
            quantize_kv_fp8(v[None], c.H, counts, out=c.v8[r:r + 1], scale_out=c.v_scale[r:r + 1])
        c.gamma[r].copy_(gamma)
        c.beta[r].copy_(beta)
        if c.gamma_p is not None:                           # PackedAct.pack's layout: [s, half, g, row, q]
            for p, row in ((c.gamma_p, gamma), (c.beta_p, beta)):
                p.data.view(p.K // 32, 2, 4, 16, 8)[:, r // 16, :, r % 16, :].copy_(row.reshape(p.K // 32, 4, 8))

    def write(self, r, th, keep, z):
        """One request into row r: th (1, keys, d), its conditioning padded to `keys` keys so that every admission
        runs one GEMM shape, keep (1, keys) bool, True = attend (counted as generate() counts it), z (1, d_style)."""
        counts = key_counts(keep)
        self.kpm[r] = ~keep[0]
        self.kv_lens[r:r + 1].copy_(counts)
        for c in self.layers:
            d = c.Wkv.shape[1]
            kv, gb = self.project_kv(c, th), self.project_film(c, z)[0]
            self._put(c, r, kv[:, :d], kv[:, d:], gb[:d], gb[d:], counts)

    def copy(self, src, r, keys=True):
        """Row src into row r (a further sample of its request): the FiLM rows and, with `keys`, mask, count, K / V."""
        if keys:
            self.kpm[r] = self.kpm[src]
            self.kv_lens[r:r + 1].copy_(self.kv_lens[src:src + 1])
        for c in self.layers:
            k, v = (None, None) if self.fp8 else (c.k[src], c.v[src])
            self._put(c, r, k, v, c.gamma[src], c.beta[src], src=src, keys=keys)

    def clear(self, r):
        """Row r idle again (what `idle` allocates), through the write path."""
        z = torch.zeros((), device=self.kpm.device, dtype=self.cd)
        for c in self.layers:
            k, f = z.expand(self.keys, c.gamma.shape[1]), z.expand(c.gamma.shape[1])
            self._put(c, r, k, k, f, f)
        self.kpm[r] = True
        self.kpm[r, 0] = False
        self.kv_lens[r:r + 1].fill_(1)
        self.point(r, r)

    def point(self, r, h):
        """Query row r reads the K/V, mask and count of row h (a share_keys session; nothing to do otherwise)."""
        if self.kv_rows is not None:
            self.kv_rows[r:r + 1].fill_(h)
