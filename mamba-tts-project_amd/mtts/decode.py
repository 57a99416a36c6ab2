"""Incremental decoding engine for MambaTTSDecoder.decode_step (C4).

Reference: mamba_decoder.py:188-256.  Each AR step embeds one token (no
quant_embed, pos = step_index), runs every layer with its Mamba state and
cross-attends to [ref ‖ text].  The reference recomputes, every step, the
K/V projections of the (constant) conditioning sequence and the FiLM
gamma/beta of the (constant) style vector; the engine computes them once per
context and keeps them in HBM (ctx.cond, the Conditioning of mtts/conditioning.py,
held by the model's cast constants, the DecodeContext of mtts/context.py, which
also decides which step runs) with the per-layer SSM/conv state.

Engine path (inference only: torch.no_grad, HIP tensors):
  * context cache keyed on the object identity (strong references are
    held, so addresses cannot be recycled) and autograd version of
    text_hidden, text_mask, ref_hidden, ref_mask, z_style, plus the compute
    dtype and batch shape;
  * per step: token+pos embedding, then per layer LN -> Mamba.step (HIP
    conv-window + state-update kernels, states updated in place) -> fused
    residual+LN -> q-projection + attention over cached K/V -> fused
    residual+LN+FiLM -> FFN; the FFN residual is fused into the next LN;
  * the <= 32-row projections (in/x/dt/out_proj, q/out_proj, FFN, head) on
    the HIP skinny GEMM of csrc/rows.hip (bias + GELU fused) for bf16;
  * dt_proj fused into the selective state update (B / C read in place);
  * a key side past the single-pass range (decode_split_chunk(hd) keys; the
    5248 keys of train.py's conditioning) on the split-key kernel
    (attention_decode_split) from every step, packed included, each row
    reading its own key count kv_lens = key_counts(keep) only;
    with generate(kv_dtype="fp8") / open_session(kv_dtype="fp8") those K / V
    are kept as OCP FP8 bytes with a scale per (row, head) (quantize_kv_fp8)
    and read by the kernel's fp8 form (attention_decode_split_fp8);
  * optional hipGraph capture of the whole step (static token / position /
    state buffers): replay costs one launch instead of ~25 per layer.
  * generate(): the loop around the step on the device -- one hipGraph of
    step + token sampler (csrc/sample.hip) replayed per token, the token,
    step and position counters never leaving HBM; a prompt prefilled through
    the scan path.  Positions are per row ((B,) device buffers), so a ragged,
    right-padded prompt batch (prompt_lengths) runs the same captured graph:
    the prefill stops every row's scan / conv state at its own length.
    Per-request sampling (per-row temperature / top-k / top-p / seed / length
    cap, repetition penalty) goes through the per-row sampler, whose controls
    are (B,) device buffers too: one graph serves every mix of settings.
  * continuous batching (mtts/session.py DecodeSession): the same step
    functions over static per-slot buffers of a private engine, finished
    rows refilled in place under one captured graph.
Numerics are those of the eager module path (tests/test_gpu_modules.py).
Call `reset()` after modifying weights in place between decode steps.
"""
from __future__ import annotations


import torch
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .embed import _err_flag, embed_sum
from .attn_kernels import attention_decode_qproj_packed, decode_split_chunk
from .conditioning import Conditioning
from .context import DecodeContext
from .linear import cast_scope


def _same_ctx(refs, versions, tensors):
    """True when `tensors` are the very objects cached in `refs` (identity,
    not address: the engine holds strong references, so a freed tensor's
    address can never be reused for a new one while the cache is alive)
    and none was modified in place since (autograd version counter)."""
    if refs is None or len(refs) != len(tensors):
        return False
    for r, v, t in zip(refs, versions, tensors):
        if r is not t:
            return False
        if t is not None and t._version != v:
            return False
    return True


def _is_scalar(v):
    """A plain number or a 0-d tensor / array (generate's per-row arguments)."""
    if isinstance(v, (list, tuple)):
        return False
    shape = getattr(v, "shape", None)
    return shape is None or len(shape) == 0


def _per_row(name, v, B, integer):
    """`v`, a scalar or (B,) list / tensor, as a (B,) CPU tensor: float64, or
    int64 when `integer` (seeds wrapped into the int64 range, as the scalar
    path does).  Raises ValueError naming the argument."""
    if isinstance(v, torch.Tensor):
        if integer and (v.dtype.is_floating_point or v.dtype == torch.bool):
            raise ValueError(f"generate: {name} must hold integers")
        v = v.detach().cpu().tolist()              # the one host copy of a device tensor
    elif hasattr(v, "tolist"):
        v = v.tolist()
    vals = list(v) if isinstance(v, (list, tuple)) else [v] * B
    if len(vals) != B:
        raise ValueError(f"generate: {name} must be a scalar or hold one value per row ({B}), got {len(vals)}")
    try:
        if integer:
            if any(isinstance(x, float) and x != int(x) for x in vals):
                raise ValueError
            vals = [(int(x) + (1 << 63)) % (1 << 64) - (1 << 63) if name == "seed" else int(x) for x in vals]
            return torch.tensor(vals, dtype=torch.int64)
        return torch.tensor([float(x) for x in vals], dtype=torch.float64)
    except (TypeError, ValueError, OverflowError, RuntimeError):
        raise ValueError(f"generate: {name} must hold {'integers' if integer else 'numbers'}") from None


def _check_window(who, window):
    if isinstance(window, bool) or not isinstance(window, int) or not 0 <= window <= 256:
        raise ValueError(f"{who}: repetition_window must be an integer in [0, 256]")


def _check_vocab_ids(who, V, pad_id, eos_id):
    if not 0 <= int(pad_id) < V or (eos_id is not None and not 0 <= int(eos_id) < V):
        raise ValueError(f"{who}: pad_id / eos_id outside the vocabulary of {V}")


def _check_request(m, B, n_new, prompt_tokens, start_token, logit_bias, pad_id, eos_id, prompt_lengths=None):
    """What generate() and a session's admit() verify of a request of B rows
    and n_new new tokens (the largest row's): the prompt's shape, its
    positions against pos_embed, pad_id / eos_id, the logit_bias shape and the
    start / prompt token ids.  Nothing is written.  Returns the prompt, its
    length Tp and `lens`: with prompt_lengths (B,) of different values the
    prompt cut at the longest row, its padding slots set to a valid id on a
    copy, and the lengths as (B,) int32 on the model's device; else None."""
    V = m.head.weight.shape[0]
    if prompt_tokens is not None and (prompt_tokens.dim() != 2 or prompt_tokens.shape[0] != B
                                      or prompt_tokens.shape[1] < 1):
        raise ValueError(f"generate: prompt_tokens must be (B, Tp) with Tp >= 1 (B = {B})")
    Tp = 1 if prompt_tokens is None else prompt_tokens.shape[1]
    lens = None
    if prompt_lengths is not None:
        if prompt_tokens is None:
            raise ValueError("generate: prompt_lengths needs prompt_tokens")
        pl = torch.as_tensor(prompt_lengths)
        if tuple(pl.shape) != (B,) or pl.dtype.is_floating_point or pl.dtype == torch.bool:
            raise ValueError(f"generate: prompt_lengths must be ({B},) integers")
        lo, hi = int(pl.min()), int(pl.max())
        if lo < 1 or hi > Tp:
            raise ValueError(f"generate: prompt_lengths must lie in [1, Tp = {Tp}] (got {lo}..{hi})")
        # columns past the longest row are padding in every row; equal lengths are a rectangular prompt
        prompt_tokens, Tp = prompt_tokens[:, :hi], hi
        if lo < hi:
            dev = m.token_embed.weight.device
            lens = pl.to(device=dev, dtype=torch.int32)
            # the padding slots' values are ignored: a valid id on a copy, before any check or embedding
            keep = torch.arange(Tp, device=dev)[None, :] < lens[:, None]
            prompt_tokens = torch.where(keep, prompt_tokens.to(dev), torch.zeros((), dtype=prompt_tokens.dtype,
                                                                                  device=dev))
    if Tp + n_new - 1 > m.pos_embed.num_embeddings:
        raise IndexError(f"generate: {Tp} prompt + {n_new} new tokens need positions beyond pos_embed "
                         f"({m.pos_embed.num_embeddings}) (index out of range in self)")
    _check_vocab_ids("generate", V, pad_id, eos_id)
    if logit_bias is not None and tuple(logit_bias.shape) not in ((V,), (B, V)):
        raise ValueError(f"generate: logit_bias must be (V,) or (B, V) (B = {B})")
    n_tok = m.token_embed.num_embeddings
    if prompt_tokens is None:
        if not 0 <= int(start_token) < n_tok:
            raise IndexError("generate: start_token out of range of token_embed (index out of range in self)")
    elif int(prompt_tokens.min()) < 0 or int(prompt_tokens.max()) >= n_tok:
        raise IndexError("generate: prompt token id out of range of token_embed (index out of range in self)")
    return prompt_tokens, Tp, lens


def check_kv_dtype(who, model, kv_dtype, n_keys):
    """kv_dtype of generate() / open_session() against a key side of n_keys
    keys: None, or "fp8", which the split-key attention alone reads.  Raises
    ValueError with the reason; touches nothing."""
    if kv_dtype is None:
        return
    if kv_dtype != "fp8":
        raise ValueError(f"{who}: kv_dtype must be None or 'fp8', got {kv_dtype!r}")
    check_split_keys(who, "kv_dtype='fp8'", model, n_keys, f"the key side of {n_keys} keys")


def check_split_keys(who, what, model, n_keys, side):
    """`what`, which the split-key attention alone serves, against `side`, the caller's words for its n_keys keys."""
    if not DecodeEngine.OPTIONS["split_keys"]:
        raise ValueError(f"{who}: {what} needs the split-key attention and DecodeEngine.OPTIONS['split_keys'] is off")
    for l in model.layers:
        ck = decode_split_chunk(l.cross_attn.embed_dim // l.cross_attn.num_heads)
        if n_keys <= ck:
            raise ValueError(f"{who}: {what} needs the split-key attention and {side} is inside the single-pass range "
                             f"(<= {ck} keys at this head dim)")


def sampler_buffers(B, V, cap, dev, logprobs=False):
    """The per-row sampler's controls and history for B rows of at most `cap`
    tokens, as device buffers a captured launch reads at run time: generate()'s
    and a decode session's.  logprobs: also `lp_hist`, the fp32 (B, cap)
    history of the emitted tokens' log-probabilities."""
    lp = dict(lp_hist=torch.zeros(B, cap, dtype=torch.float32, device=dev)) if logprobs else {}
    return dict(lp, temperature=torch.zeros(B, dtype=torch.float32, device=dev),
                top_k=torch.zeros(B, dtype=torch.int32, device=dev),
                top_p=torch.ones(B, dtype=torch.float32, device=dev),
                row_seed=torch.zeros(B, dtype=torch.int64, device=dev),
                draw=torch.zeros(B, dtype=torch.int32, device=dev),
                penalty=torch.ones(B, dtype=torch.float32, device=dev),
                max_length=torch.full((B,), cap, dtype=torch.int64, device=dev),
                hist=torch.zeros(B, cap, dtype=torch.int64, device=dev),
                unfinished=torch.zeros(1, dtype=torch.int32, device=dev),
                bias=torch.zeros(B, V, dtype=torch.float32, device=dev))


def capture_graph(body, restore):
    """`body` as a hipGraph: two warm-up runs on a side stream (allocator,
    library handles, lazily made workspaces), `restore()` before each of them,
    before the capture and after it, so the buffers `body` advances are left
    as `restore` makes them.  Returns the graph and what the captured `body`
    returned (its static output)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            restore()
            body()
    torch.cuda.current_stream().wait_stream(s)
    restore()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = body()
    restore()
    return g, out


BLAS_ROWS = 32   # with log-probabilities: the generic step's projections of fewer rows run as this many


def _proj_blas(x, w, b=None, act=None, rows=0):
    """A projection of the generic step on the BLAS GEMM.  The library picks
    its tiling, and with it the order of every sum, by the GEMM's shape, so a
    row's result depends on how many rows share the step (measured: the fp32
    logits of one request differ by 2e-6 between 20 rows and 1).  `rows` > 0
    (generate(return_logprobs=True) and sessions opened with logprobs=True
    only): fewer rows than that run as exactly `rows`, zero rows appended --
    one shape, so a request's logits, and the log-probabilities made of them,
    are the same bits in a session of any size and in generate() on the
    request alone, as on the fused step.  It costs one pad launch per
    projection (profiles/sample_logprobs_ab.txt).  Every other caller passes
    0 and runs the GEMM as it comes, as before."""
    M = x.shape[0]
    if M < rows:
        x = F.pad(x, (0, 0, 0, rows - M))
    y = x @ w.t() if b is None else torch.addmm(b, x, w.t())
    y = F.gelu(y) if act == "gelu" else y
    return y[:M] if M < rows else y


def _proj_rows(x, w, b=None, act=None, rows=0):
    """HIP skinny GEMM (csrc/rows.hip) for the <= 32-row decode projections."""
    if ops.gemm_rows_ok(x, w):
        return ops.gemm_rows(x, w, b, act)
    return _proj_blas(x, w, b, act, rows)


class DecodeEngine:
    # routing switches for in-process A/B timing (tools/decode_ab.py); the
    # defaults are the measured-fastest path (DESIGN.md §4 decode)
    OPTIONS = {"rows": True,       # HIP row-GEMMs (csrc/rows.hip / gemv.hip) instead of hipBLASLt
               "fused": True,      # fused-epilogue step (LN prologues, residual / conv epilogues)
               "fuse_conv": True,  # conv update in in_proj's epilogue
               "packed": True,     # weights re-laid in MFMA fragment order (gemv16)
               "xpacked": True,    # activation images packed too
               # cross-attention LN + q projection inside the decode attention kernel
               # (mtts_attention_decode_qproj): measured 1.13 vs 0.76 ms p50 per
               # step (profiles/r05_decode_ab_fuse_q.txt) -- every (batch, head)
               # workgroup re-reads its head's Wq rows (256 KiB) from L2, 64 MiB
               # per layer against 2 MiB for one projection over the 32 rows
               "fuse_q": False,
               # key sides past the single-pass range (decode_split_chunk(hd) keys) on the
               # split-key kernel (mtts_attention_decode_split), which keeps the packed
               # step on and reads a row's own key count only; off: the serial
               # attn_decode_kernel under the unpacked step (profiles/decode_long_keys.txt)
               "split_keys": True}

    def __init__(self, model, use_graph=True, use_rows=True):
        self.m = model
        self.use_graph = use_graph
        self.use_rows = use_rows and self.OPTIONS["rows"]
        self.reset()

    def reset(self):
        # a flag left by the previous session must not surface in the next one,
        # and must not be lost either (nn.Embedding raises on every such step,
        # mamba_decoder.py:217): wait for its copy, clear host and device
        # flags, reset the engine, then raise it
        flagged = False
        if getattr(self, "_err_ev", None) is not None:
            self._err_ev.synchronize()
            flagged = int(self._err_host[0]) != 0
            self._err_host.zero_()
            _err_flag(self._err_dev).zero_()
        self._err_host = None
        self._err_ev = None
        self._err_dev = None
        self.drop()
        if flagged:
            raise IndexError("decode_step: last_token id out of range of token_embed (index out of range in self)")

    # -- the context and what lives as long as it does ----------------------------
    def drop(self):
        """No context: everything whose lifetime is the context's, declared here and nowhere else."""
        self.ctx = None                                     # the DecodeContext (adopt)
        self.ctx_key = self.ctx_refs = self.ctx_versions = None     # what _prepare built it from
        self.states = self.tok_buf = self.pos_buf = self.pos32 = None   # the static buffers (adopt)
        self.graph = self.out_buf = None                    # decode_step's capture and its static output
        self.gen_graphs = {}                                # generate's captures, its buffers, its prefill's logits
        self.gen = self.prefill_logits = None

    def adopt(self, ctx, rows, dev):
        """`ctx` (DecodeContext.build) as the engine's context, with the static per-layer (conv, SSM) states and
        token / position buffers of `rows` rows, zeroed.  A session's prefill engine adopts the stepping
        engine's context at 1 row: the constants and the routing are shared, the states are its own."""
        self.ctx = ctx
        self.states = [(torch.zeros(rows, l.mamba.d_inner, l.mamba.d_conv, device=dev),
                        torch.zeros(rows, l.mamba.d_inner, l.mamba.d_state, device=dev)) for l in self.m.layers]
        self.tok_buf = torch.zeros(rows, 1, dtype=torch.long, device=dev)
        # per-row positions: int64 for the eager step's F.embedding, int32 for the fused step
        self.pos_buf = torch.zeros(rows, dtype=torch.long, device=dev)
        self.pos32 = torch.zeros(rows, dtype=torch.int32, device=dev)

    @property
    def step_pos(self):
        """The position buffer the step reads: the fused step embeds int32 position ids."""
        return self.pos32 if self.ctx.fused else self.pos_buf

    def set_pos(self, value, rows=slice(None)):
        """Both position buffers, on `rows`, from an int or a tensor."""
        for buf in (self.pos32, self.pos_buf):
            if isinstance(value, torch.Tensor):
                buf[rows].copy_(value)
            else:
                buf[rows].fill_(value)

    def _embed(self, tok):
        """token_embed(last_token) + pos_embed(step_index) in the compute dtype
        (mamba_decoder.py:188-256; no quant_embed in decode_step) as ONE
        mtts_embed_sum_at launch (a zero quantizer row, each row's position id
        from the (B,) int32 buffer pos32) instead of two gathers, an add and a
        cast."""
        m, c = self.m, self.ctx
        B = c.rows
        d = m.token_embed.weight.shape[1]
        out = torch.empty(B, d, device=tok.device, dtype=c.cd)
        tw, pw = c.tok_w, c.pos_w
        L.call_raw("mtts_embed_sum_at", tok.data_ptr(), tok.stride(0), c.q0_id.data_ptr(), self.pos32.data_ptr(),
                   tw.data_ptr(), c.q0_w.data_ptr(), pw.data_ptr(), B, 1, d, tw.shape[0], out.data_ptr(),
                   L.dtype_code(out), out.stride(0), _err_flag(tok.device).data_ptr(), 1, pw.shape[0])
        return out

    # -- one step, fused epilogues (bf16, <= 32 sequences) ---------------------
    def _step_rows(self, tok, pos, states):
        """Per layer, 9 launches and no LayerNorm kernel (csrc/rows.hip):
        in_proj (LN prologue, conv-update + SiLU epilogue) -> x_proj ->
        state update (+dt_proj) -> out_proj (+residual) -> q (LN prologue)
        -> attention -> out_proj (+residual) -> FFN up (LN + FiLM prologue,
        GELU) -> FFN down (+residual); the head LayerNorms in its prologue.
        x is the bf16 residual stream, exactly as the LayerNorm kernels'
        x_sum of the generic step."""
        m, c = self.m, self.ctx
        cond = c.cond
        x = self._embed(tok)

        def ln(norm, gamma=None, beta=None):
            return (norm.weight, norm.bias, norm.eps, gamma, beta)

        if c.xpk:
            return self._step_xpk(x, states, ln)

        fuse_conv = self.OPTIONS["fuse_conv"]
        for i, (l, p, cl) in enumerate(zip(m.layers, c.layers, cond.layers)):
            conv_state, ssm_state = states[i]
            mm = l.mamba
            di, N, r = mm.d_inner, mm.d_state, mm.dt_rank
            if fuse_conv:
                xz, u = ops.gemm_rows(x, p.Win.operand, conv=(conv_state, p.conv_w, p.conv_b),
                                      ln=ln(l.norm_mamba))
            else:
                xz = ops.gemm_rows(x, p.Win.operand, ln=ln(l.norm_mamba))
                u = ops.conv_update(xz[:, :di], conv_state, p.conv_w, p.conv_b, True)
            x_dbl = ops.gemm_rows(u, p.Wx.operand)
            y = ops.state_update(ssm_state, u, x_dbl[:, :r], p.A, x_dbl[:, r:r + N], x_dbl[:, r + N:], p.D,
                                 xz[:, di:], p.dt_bias, True, dt_w=p.Wdt)
            x = ops.gemm_rows(y, p.Wout.operand, res=x)
            q = ops.gemm_rows(x, p.Wq.operand, p.bq, ln=ln(l.norm_cross))
            o = cond.attend(cl, q, packed=False)
            x = ops.gemm_rows(o, p.Wo.operand, p.bo, res=x)
            f = ops.gemm_rows(x, p.W1.operand, p.b1, "gelu", ln=ln(l.norm_ff, cl.gamma, cl.beta))
            x = ops.gemm_rows(f, p.W2.operand, p.b2, res=x)
        return ops.gemm_rows(x, c.Wh.operand, c.bh, ln=ln(m.norm_out))[:, None]

    def _step_xpk(self, x, states, ln):
        """_step_rows with packed activations (csrc/gemv.hip, common.h
        xpk_index): every producer writes the packed image of what the next
        projection reads (residual epilogues the residual stream besides its
        row-major copy, the conv-update u for x_proj, the state-update y for
        out_proj, attention o, FFN-up f) and the FiLM rows are packed once
        per context, so every projection loads its operands as coalesced KiB
        like its weights; the LayerNorm(+FiLM) prologues run on the packed
        rows.  9 launches per layer, as _step_rows."""
        m, c = self.m, self.ctx
        cond = c.cond
        xp = None   # packed image of the residual stream (none before layer 0)
        for i, (l, p, cl) in enumerate(zip(m.layers, c.layers, cond.layers)):
            conv_state, ssm_state = states[i]
            mm = l.mamba
            di, N, r = mm.d_inner, mm.d_state, mm.dt_rank
            xz, u, up = ops.gemm_rows(x if xp is None else xp, p.Win.packed,
                                      conv=(conv_state, p.conv_w, p.conv_b), ln=ln(l.norm_mamba),
                                      u_packed=True)
            # (x_proj fused into the state update measured slower, 1.10 vs 0.77 ms
            # per step: every workgroup pulls 512 KiB through dependent L2 trips)
            x_dbl = ops.gemm_rows(up, p.Wx.packed)
            y = ops.state_update(ssm_state, u, x_dbl[:, :r], p.A, x_dbl[:, r:r + N], x_dbl[:, r + N:], p.D,
                                 xz[:, di:], p.dt_bias, True, dt_w=p.Wdt, packed_out=True)
            x, xp = ops.gemm_rows(y, p.Wout.packed, res=x, packed_out="also")
            if c.fuse_q:   # one launch: LN + q projection in the attention kernel's prologue
                nc = l.norm_cross
                o = attention_decode_qproj_packed(x, p.Wq.w, p.bq, nc.weight, nc.bias, nc.eps, cl.khm, cl.vhm,
                                                  cl.H, cond.kpm)
            else:
                q = ops.gemm_rows(xp, p.Wq.packed, p.bq, ln=ln(l.norm_cross))
                o = cond.attend(cl, q, packed=True)
            x, xp = ops.gemm_rows(o, p.Wo.packed, p.bo, res=x, packed_out="also")
            f = ops.gemm_rows(xp, p.W1.packed, p.b1, "gelu", ln=ln(l.norm_ff, cl.gamma_p, cl.beta_p),
                              packed_out="only")
            x, xp = ops.gemm_rows(f, p.W2.packed, p.b2, res=x, packed_out="also")
        return ops.gemm_rows(xp, c.Wh.packed, c.bh, ln=ln(m.norm_out))[:, None]

    def step_fn(self, logprobs):
        """The step generate() and a session run: the fused step, or the
        generic one -- with log-probabilities asked for, its BLAS projections
        at BLAS_ROWS rows, so that the values do not depend on the row count;
        without, exactly as decode_step runs it."""
        if self.ctx.fused:
            return self._step_rows
        if not logprobs:
            return self._step
        return lambda tok, pos, states: self._step(tok, pos, states, rows=BLAS_ROWS)

    # -- one step, eager -----------------------------------------------------
    def _step(self, tok, pos, states, rows=0):
        m, c = self.m, self.ctx
        cd, cond = c.cd, c.cond
        x = (F.embedding(tok, m.token_embed.weight) + F.embedding(pos, m.pos_embed.weight)[:, None]).to(cd)
        x = x.view(c.rows, -1)                                               # (B, d)
        proj = _proj_rows if (self.use_rows and cd == torch.bfloat16) else _proj_blas

        def mm_(x, w, b=None, act=None):   # rows > 0: the BLAS projections at that fixed row count (_proj_blas)
            return proj(x, w, b, act, rows)
        pending = None
        for i, (l, p, cl) in enumerate(zip(m.layers, c.layers, cond.layers)):
            conv_state, ssm_state = states[i]
            h, xs = ops.layer_norm(x if pending is None else pending, l.norm_mamba.weight, l.norm_mamba.bias,
                                   l.norm_mamba.eps, res=None if pending is None else x)
            if pending is not None:
                x = xs
            mm = l.mamba
            di, N, r = mm.d_inner, mm.d_state, mm.dt_rank
            xz = mm_(h, p.Win.w)
            u = ops.conv_update(xz[:, :di], conv_state, p.conv_w, p.conv_b, True)
            x_dbl = mm_(u, p.Wx.w)
            # dt_proj fused into the state update; B / C read in place from x_dbl
            y = ops.state_update(ssm_state, u, x_dbl[:, :r], p.A, x_dbl[:, r:r + N], x_dbl[:, r + N:], p.D,
                                 xz[:, di:], p.dt_bias, True, dt_w=p.Wdt)
            h_m = mm_(y, p.Wout.w)
            h, x = ops.layer_norm(h_m, l.norm_cross.weight, l.norm_cross.bias, l.norm_cross.eps, res=x)
            q = mm_(h, p.Wq.w, p.bq)
            o = cond.attend(cl, q, packed=False)
            a = mm_(o, p.Wo.w, p.bo)
            h, x = ops.layer_norm(a, l.norm_ff.weight, l.norm_ff.bias, l.norm_ff.eps, res=x,
                                  gamma=cl.gamma, beta=cl.beta, rows_per_group=1)
            pending = mm_(mm_(h, p.W1.w, p.b1, "gelu"), p.W2.w, p.b2)
        h, _ = ops.layer_norm(pending, m.norm_out.weight, m.norm_out.bias, m.norm_out.eps, res=x)
        return mm_(h, c.Wh.w, c.bh)[:, None]

    # -- out-of-range token ids --------------------------------------------------
    def _check_token_flag(self, dev, blocking=False):
        """The fused step embeds through mtts_embed_sum, which zero-fills and
        flags a row whose token id is outside token_embed (nn.Embedding raises
        there, mamba_decoder.py:217).  The flag of an earlier step is read from
        a pinned copy; without `blocking` only once its event has completed (no
        host sync), so the IndexError is best-effort and deferred: it comes at
        a later decode_step once the GPU has caught up, or at check_errors(),
        which waits for the copy and is the guarantee."""
        if self._err_ev is None:
            return
        if blocking:
            self._err_ev.synchronize()
        elif not self._err_ev.query():
            return
        if int(self._err_host[0]) != 0:
            self._err_host.zero_()
            _err_flag(dev).zero_()
            raise IndexError("decode_step: last_token id out of range of token_embed (index out of range in self)")

    def check_errors(self):
        """Blocking: raise IndexError if any step since the last check embedded
        an out-of-range token id (call before reset() / at the end of a
        generation to observe every error)."""
        if self._err_dev is not None:
            self._check_token_flag(self._err_dev, blocking=True)

    def _post_token_flag(self, dev):
        if self._err_host is None:
            self._err_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            self._err_ev = torch.cuda.Event()
            self._err_dev = dev
        self._err_host.copy_(_err_flag(dev), non_blocking=True)
        self._err_ev.record()

    def _prepare(self, conds, tok_shape, dev, kv_dtype=None):
        """Conditioning context (rebuilt when `conds`, the compute dtype, the
        token shape or kv_dtype changed; every graph goes with it) and the
        static state / token / position buffers."""
        m = self.m
        cd = m._cd()
        key = (cd, tok_shape) if kv_dtype is None else (cd, tok_shape, kv_dtype)
        B = tok_shape[0]
        if key != self.ctx_key or not _same_ctx(self.ctx_refs, self.ctx_versions, conds):
            self.drop()
            # the split-key routing is latched here, with the conditioning: the context's latch and every step agree
            cond = Conditioning.from_batch(m, *conds, cd, kv_dtype, self.OPTIONS["split_keys"])
            self.adopt(DecodeContext.build(m, cond, B, self.use_rows), B, dev)
            self.ctx_key = key
            self.ctx_refs = conds                  # strong references (see _same_ctx)
            self.ctx_versions = tuple(None if t is None else t._version for t in conds)

    # -- public ----------------------------------------------------------------
    @torch.no_grad()
    def step(self, last_token, text_hidden, z_style, mamba_states, step_index, text_mask=None, ref_hidden=None,
             ref_mask=None):
        m = self.m
        self._check_token_flag(last_token.device)
        B = last_token.shape[0]
        dev = last_token.device
        self._prepare((text_hidden, z_style, text_mask, ref_hidden, ref_mask), tuple(last_token.shape), dev)
        # adopt the caller's states (None = start of sequence)
        for i, st in enumerate(self.states):
            given = None if mamba_states is None else mamba_states[i]
            if given is None:
                st[0].zero_()
                st[1].zero_()
            elif given[0] is not st[0] or given[1] is not st[1]:
                st[0].copy_(given[0])
                st[1].copy_(given[1])
        self.tok_buf.copy_(last_token)
        pbuf = self.step_pos                                # this one alone: the timed loop gets no second launch
        if isinstance(step_index, torch.Tensor) and step_index.dim() > 0:   # per-row positions
            if tuple(step_index.shape) != (B,) or step_index.dtype.is_floating_point or step_index.dtype == torch.bool:
                raise ValueError(f"decode_step: a tensor step_index must be ({B},) integers, one position per row")
            if not (0 <= int(step_index.min()) and int(step_index.max()) < m.pos_embed.num_embeddings):
                raise IndexError("index out of range in self")
            pbuf.copy_(step_index)
        else:
            if not 0 <= int(step_index) < m.pos_embed.num_embeddings:   # pos_embed(step_index) raises (:226)
                raise IndexError("index out of range in self")
            pbuf.fill_(int(step_index))
        step = self._step_rows if self.ctx.fused else self._step
        if not self.use_graph:
            logits = step(self.tok_buf, self.pos_buf, self.states)
            if self.ctx.fused:
                self._post_token_flag(dev)
            return logits, list(self.states)
        if self.graph is None:
            saved = [(a.clone(), b.clone()) for a, b in self.states]

            def restore():   # the warm-up runs advanced the states
                for (a, b), (sa, sb) in zip(self.states, saved):
                    a.copy_(sa)
                    b.copy_(sb)

            self.graph, self.out_buf = capture_graph(lambda: step(self.tok_buf, self.pos_buf, self.states), restore)
        self.graph.replay()
        if self.ctx.fused:
            self._post_token_flag(dev)
        return self.out_buf.clone(), list(self.states)

    # -- generation ------------------------------------------------------------
    def _gen_buffers(self, B, V, dev, logprobs=False):
        """Device-resident generation state, made once per context (before any
        capture): seed / step counters, the token history, end-of-sequence
        bookkeeping, the logit bias, pinned slots for the early-stop polls and
        the per-row sampler's controls (filled per call, read at run time).
        The log-probability history joins them at the first call that asks
        for it, before that call's capture."""
        cap = self.m.pos_embed.num_embeddings
        if self.gen is not None and logprobs and "lp_hist" not in self.gen:
            self.gen["lp_hist"] = sampler_buffers(B, V, cap, dev, logprobs=True)["lp_hist"]
        if self.gen is None:
            self.gen = dict(
                sampler_buffers(B, V, cap, dev, logprobs),
                seed=torch.zeros(1, dtype=torch.int64, device=dev), step=torch.zeros(1, dtype=torch.int32, device=dev),
                finished=torch.zeros(B, dtype=torch.int32, device=dev),
                length=torch.zeros(B, dtype=torch.int64, device=dev),
                host=torch.zeros(cap, dtype=torch.int32, pin_memory=True))
        return self.gen

    @staticmethod
    def _row_controls(B, temperature, top_k, top_p, seed, max_new_tokens, penalty, window):
        """generate's per-row arguments, scalars broadcast, checked on the host
        (ValueError names the argument) and returned as (B,) CPU tensors under
        the names of the device buffers they fill, plus the window."""
        T = _per_row("temperature", temperature, B, False)
        k = _per_row("top_k", top_k, B, True)
        p = _per_row("top_p", top_p, B, False)
        caps = _per_row("max_new_tokens", max_new_tokens, B, True)
        th = _per_row("repetition_penalty", 1.0 if penalty is None else penalty, B, False)
        if _is_scalar(seed):
            s = torch.tensor(ops.row_seeds(int(seed), B), dtype=torch.int64)
        else:
            s = _per_row("seed", seed, B, True)
        if not bool((torch.isfinite(T) & (T >= 0)).all()):
            raise ValueError("generate: temperature must be finite and >= 0 in every row")
        if not bool(((k >= 0) & (k < (1 << 31))).all()):
            raise ValueError("generate: top_k must be >= 0 in every row")
        if not bool(((p > 0) & (p <= 1)).all()):
            raise ValueError("generate: top_p must be in (0, 1] in every row")
        if not bool((torch.isfinite(th) & (th > 0)).all()):
            raise ValueError("generate: repetition_penalty must be finite and > 0 in every row")
        if not bool((caps >= 1).all()):
            raise ValueError("generate: max_new_tokens must be >= 1 in every row")
        _check_window("generate", window)
        return dict(temperature=T.float(), top_k=k.int(), top_p=p.float(), row_seed=s, penalty=th.float(),
                    max_length=caps, window=window)

    def _prefill(self, prompt, conds, lens=None):
        """The whole prompt through the parallel (scan) path: one embed_sum
        with a zero quantizer row (decode_step adds no quant_embed,
        mamba_decoder.py:217-221), the layer stack from empty states, the head
        on the last position.  The per-layer (conv_state, ssm_state) it returns
        become the engine's states; returns the last position's logits (B, V).
        `lens` (B,) int32 on the device: the prompt is ragged and right-padded;
        every layer's scan and conv state stop at the row's own length and the
        head reads the row's position lens[b] - 1."""
        m, c = self.m, self.ctx
        text_hidden, z_style, text_mask, ref_hidden, ref_mask = conds
        cd = c.cd
        B, Tp = prompt.shape
        th = text_hidden.to(cd)
        th, tm = m._concat_ref(th, text_mask, ref_hidden, ref_mask, B, th.device)
        qid = torch.zeros(Tp, dtype=torch.long, device=prompt.device)
        x = embed_sum(prompt, qid, m.token_embed.weight, c.q0_w, m.pos_embed.weight, cd)
        with cast_scope(m._gemm_weights(), cd):
            if lens is None:
                x, pending, new_states = m._run_layers(x, th, z_style, tm, None)
                last = lambda t: t[:, -1:].contiguous()  # noqa: E731
            else:
                x, pending, new_states = m._run_layers(x, th, z_style, tm, None, seq_lens=lens)
                rows, at = torch.arange(B, device=prompt.device), lens.long() - 1
                last = lambda t: t[rows, at][:, None].contiguous()  # noqa: E731
            logits = m._tail(last(x), None if pending is None else last(pending))
        for (cs, ss), (ncs, nss) in zip(self.states, new_states):
            cs.copy_(ncs)
            ss.copy_(nss)
        return logits[:, 0]

    @torch.no_grad()
    def generate(self, text_hidden, z_style, max_new_tokens, prompt_tokens=None, start_token=0, text_mask=None,
                 ref_hidden=None, ref_mask=None, temperature=1.0, top_k=0, top_p=1.0, logit_bias=None, eos_id=None,
                 pad_id=0, seed=0, check_every=32, prompt_lengths=None, repetition_penalty=None,
                 repetition_window=64, return_logprobs=False, kv_dtype=None):
        """Autoregressive generation on the device: each new token is one
        replay of a hipGraph holding the decode step and the sampler
        (csrc/sample.hip), which writes the token buffer the next step embeds,
        the history column and the end-of-sequence bookkeeping, and advances
        the step / position counters -- no per-token copy, fill, clone or
        error-flag read on the host.  A prompt longer than one token is
        prefilled through the scan path (_prefill) and its last logits feed
        the first draw; prompt tokens sit at positions 0..Tp-1, new token i is
        drawn from the logits at position Tp-1+i and fed at Tp+i.
        With prompt_lengths (B,), 1 <= len_b <= Tp, the prompt is ragged and
        right-padded: one prefill over (B, max len) with per-row lengths, row
        b's positions start at len_b - 1 and move in lockstep from there, and
        new token i of every row is history column i.  Positions are device
        data, so ragged and rectangular calls replay the same graph.

        The seed lives in device memory (a new seed replays the same graph);
        temperature / top_k / top_p / eos_id / pad_id key the graph cache.
        With eos_id, every `check_every` steps the unfinished-row count is
        copied to pinned memory without blocking and the previous poll is
        waited for (so the host runs at most two polls ahead of the GPU);
        generation stops once a poll reads 0.  The engine's state buffers are
        reused: a decode_step sequence in flight on this engine does not
        survive a generate call (a following one, from step 0, does).

        Per-request sampling: temperature, top_k, top_p, seed and
        max_new_tokens each take a scalar or one value per row ((B,) list or
        tensor), and repetition_penalty (scalar or (B,); None: off) divides
        the positive and multiplies the other logits of every token among the
        row's last `repetition_window` (0..256) GENERATED tokens -- the
        history buffer; prompt tokens are not penalised.  With all of the
        former scalar and no penalty the call runs exactly as described above
        (the scalar sampler, its graph key, its tokens).  Otherwise the
        per-row sampler (ops.sample_tokens_rows) draws: its controls are (B,)
        device buffers filled per call, so the graph is keyed on ("rows",
        eos_id, pad_id, repetition_window) alone and no per-row value captures
        again.  Row b's random stream is a function of (seed_b, tokens row b
        has drawn so far, v): the same request draws the same tokens in any
        row of any batch.  A scalar seed becomes ops.row_seeds(seed, B).  A
        row stops at its own max_new_tokens (pad_id afterwards); the loop runs
        to the largest, and the early-stop poll also runs when the caps differ.

        return_logprobs: the sampler launch also records, next to every token,
        the log-probability the model gave it (include/mtts.h,
        MttsSampleLogprobOut: after logit_bias and the repetition penalty, at
        temperature 1, before top-k / top-p), the first draw from a prompt's
        prefill logits included.  Such a call has graphs of its own (the key
        gains one element); without the flag nothing differs from before.
        On the generic (non-fused) step a call with the flag runs the BLAS
        projections at a fixed row count (_proj_blas, step_fn), so that the
        values do not depend on the batch size; its logits then differ from
        those of a call without the flag by rounding (order 1e-6), and a token
        can differ where two candidates are that close.  On the fused bf16
        step both calls compute the same bits.

        kv_dtype="fp8" (None: off, and nothing differs from before): the
        conditioning K / V of every layer are kept as OCP FP8 (e4m3fn) bytes
        with one fp32 scale per (row, head), quantised once when the context
        is built (quantize_kv_fp8, over each row's key count), and every
        decode step reads them through the fp8 form of the split-key
        attention: half the K/V bytes per token.  No bf16 image of K / V is
        kept.  The value is part of the context key: a change rebuilds the
        context and its graphs.  The prompt prefill is the training-path
        attention over the unquantised conditioning and stays so, in a session
        as here, so the two agree.  ValueError when a layer's key side is
        inside the single-pass range (latency-bound there: no fp8 kernel),
        when OPTIONS["split_keys"] is off, or for any other value.
        decode_step never quantises.

        Returns tokens (B, n) int64, n <= max(max_new_tokens), and lengths (B,);
        with return_logprobs also logprobs (B, n) fp32, 0.0 at and past a row's
        length."""
        m = self.m
        V = m.head.weight.shape[0]
        B = text_hidden.shape[0]
        dev = text_hidden.device
        check_kv_dtype("generate", m, kv_dtype,
                       text_hidden.shape[1] + (0 if ref_hidden is None else ref_hidden.shape[1]))
        per_row = (repetition_penalty is not None
                   or not all(_is_scalar(v) for v in (temperature, top_k, top_p, seed, max_new_tokens)))
        ctl = None
        if per_row:
            ctl = self._row_controls(B, temperature, top_k, top_p, seed, max_new_tokens, repetition_penalty,
                                     repetition_window)
            n_new = int(ctl["max_length"].max())
        else:
            n_new = int(max_new_tokens)
        if n_new < 1 or int(check_every) < 1:
            raise ValueError("generate: max_new_tokens and check_every must be >= 1")
        if not per_row:
            if not 0 < top_p <= 1:
                raise ValueError("generate: top_p must be in (0, 1]")
            if temperature < 0 or top_k < 0:
                raise ValueError("generate: temperature and top_k must be >= 0")
        prompt_tokens, Tp, lens = _check_request(m, B, n_new, prompt_tokens, start_token, logit_bias, pad_id, eos_id,
                                                 prompt_lengths)
        self.check_errors()                         # a flag left by earlier decode_steps is theirs
        conds = (text_hidden, z_style, text_mask, ref_hidden, ref_mask)
        self._prepare(conds, (B, 1), dev, kv_dtype)
        g = self._gen_buffers(B, V, dev, bool(return_logprobs))
        stepfn, fused, pos = self.step_fn(bool(return_logprobs)), self.ctx.fused, self.step_pos
        eos = None if eos_id is None else int(eos_id)

        def draw(logits):
            common = dict(logit_bias=g["bias"], step=g["step"], advance=True, out=self.tok_buf, history=g["hist"],
                          eos_id=eos, pad_id=int(pad_id), finished=g["finished"], length=g["length"],
                          unfinished=g["unfinished"], pos=pos if fused else None)
            if return_logprobs:
                common["logprob_history"] = g["lp_hist"]
            if per_row:
                ops.sample_tokens_rows(logits, temperature=g["temperature"], top_k=g["top_k"], top_p=g["top_p"],
                                       seed=g["row_seed"], draw=g["draw"], penalty=g["penalty"],
                                       window=ctl["window"], max_length=g["max_length"], **common)
            else:
                ops.sample_tokens(logits, temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                                  seed=g["seed"], **common)
            if not fused:                           # the sampler advances the fused step's int32 positions only
                pos.add_(1)

        def body():
            draw(stepfn(self.tok_buf, self.pos_buf, self.states)[:, 0])

        def rewind():
            for t in (self.tok_buf, self.pos_buf, self.pos32, g["step"], g["finished"], g["length"], g["draw"]):
                t.zero_()
            for cs, ss in self.states:
                cs.zero_()
                ss.zero_()

        run = body
        if self.use_graph:
            key = (("rows", eos, int(pad_id), ctl["window"]) if per_row
                   else (float(temperature), int(top_k), float(top_p), eos, int(pad_id)))
            if return_logprobs:
                key += ("logprobs",)
            gr = self.gen_graphs.get(key)
            if gr is None:
                g["bias"].zero_()
                gr = self.gen_graphs[key] = capture_graph(body, rewind)[0]
            run = gr.replay
        # this call's state
        rewind()
        g["unfinished"].fill_(B)
        poll = eos is not None
        if not per_row:
            g["seed"].fill_((int(seed) + (1 << 63)) % (1 << 64) - (1 << 63))
        else:
            for name in ("temperature", "top_k", "top_p", "row_seed", "penalty", "max_length"):
                g[name].copy_(ctl[name])
            poll = poll or int(ctl["max_length"].min()) < n_new
        if logit_bias is None:
            g["bias"].zero_()
        else:
            g["bias"].copy_(logit_bias.to(torch.float32).expand(B, V))
        issued = 0
        if Tp > 1:
            logits0 = self._prefill(prompt_tokens.long(), conds, lens)
            self.prefill_logits = logits0
            self.set_pos(Tp - 1 if lens is None else lens - 1)  # row b continues from its own last prompt position
            draw(logits0)                           # token 0 from the prompt's last logits; pos -> Tp
            issued = 1
        elif prompt_tokens is not None:
            self.tok_buf.copy_(prompt_tokens)
        else:
            self.tok_buf.fill_(int(start_token))
        polls, prev = 0, None
        while issued < n_new:
            run()
            issued += 1
            if poll and issued % int(check_every) == 0 and issued < n_new:
                g["host"][polls:polls + 1].copy_(g["unfinished"], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                if prev is not None:
                    prev.synchronize()
                    if int(g["host"][polls - 1]) == 0:
                        break
                prev = ev
                polls += 1
        if self.ctx.fused:
            self._post_token_flag(dev)
        torch.cuda.current_stream().synchronize()
        self.check_errors()
        lengths = g["length"].clone()
        n = issued
        if poll and int(g["unfinished"].item()) == 0:
            n = int(lengths.max())                  # trimmed at the step where every row had finished
        if return_logprobs:
            return g["hist"][:, :n].clone(), lengths, g["lp_hist"][:, :n].clone()
        return g["hist"][:, :n].clone(), lengths
