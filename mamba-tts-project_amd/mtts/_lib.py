"""ctypes binding of libmtts.so (include/mtts.h).

The library is the product: there is no CPU fallback.  Loading fails loudly
when libmtts.so is missing, and every wrapper raises RuntimeError with
mtts_last_error() on a non-zero return code.

torch must be imported before the library is loaded so that the HIP runtime
torch bundles (libamdhip64.so.7) is the one the library binds to.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTTS_LIB", os.path.join(_HERE, "libmtts.so"))
ABI_VERSION = 15

F32, BF16 = 0, 1
i32, i64, f32, vp = C.c_int, C.c_int64, C.c_float, C.c_void_p


class ScanFwdArgs(C.Structure):
    _fields_ = [("batch", i32), ("dim", i32), ("seqlen", i32), ("dstate", i32),
                ("dtype_io", i32), ("dtype_bc", i32), ("delta_softplus", i32), ("ckpt_chunk", i32),
                ("a_is_log", i32), ("reserved_", i32), ("u_bs", i64), ("u_ls", i64), ("delta_bs", i64), ("delta_ls", i64),
                ("z_bs", i64), ("z_ls", i64), ("out_bs", i64), ("out_ls", i64),
                ("B_bs", i64), ("B_ls", i64), ("C_bs", i64), ("C_ls", i64),
                ("u", vp), ("delta", vp), ("A", vp), ("Bm", vp), ("Cm", vp), ("D", vp), ("z", vp),
                ("delta_bias", vp), ("h0", vp), ("out", vp), ("last_state", vp), ("ckpt", vp),
                ("workspace", vp), ("seqlens", vp)]


class ScanBwdArgs(C.Structure):
    _fields_ = [("f", ScanFwdArgs), ("dout", vp), ("dout_bs", i64), ("dout_ls", i64),
                ("du", vp), ("du_bs", i64), ("du_ls", i64),
                ("ddelta", vp), ("ddelta_bs", i64), ("ddelta_ls", i64),
                ("dz", vp), ("dz_bs", i64), ("dz_ls", i64),
                ("dB", vp), ("dB_bs", i64), ("dB_ls", i64),
                ("dC", vp), ("dC_bs", i64), ("dC_ls", i64),
                ("dA", vp), ("dD", vp), ("ddelta_bias", vp), ("dh0", vp), ("workspace", vp)]


class ConvFwdArgs(C.Structure):
    _fields_ = [("batch", i32), ("dim", i32), ("seqlen", i32), ("width", i32), ("dtype", i32), ("silu", i32),
                ("x_bs", i64), ("x_ls", i64), ("out_bs", i64), ("out_ls", i64),
                ("x", vp), ("w", vp), ("bias", vp), ("conv_state_in", vp), ("out", vp), ("conv_state_out", vp),
                ("seqlens", vp)]


class ConvBwdArgs(C.Structure):
    _fields_ = [("f", ConvFwdArgs), ("dout", vp), ("dout_bs", i64), ("dout_ls", i64),
                ("dx", vp), ("dx_bs", i64), ("dx_ls", i64), ("dw", vp), ("dbias", vp), ("workspace", vp)]


class ConvUpdateArgs(C.Structure):
    _fields_ = [("batch", i32), ("dim", i32), ("width", i32), ("dtype", i32), ("silu", i32),
                ("x_bs", i64), ("out_bs", i64), ("x", vp), ("conv_state", vp), ("w", vp), ("bias", vp),
                ("out", vp)]


class StateUpdateArgs(C.Structure):
    _fields_ = [("batch", i32), ("dim", i32), ("dstate", i32), ("dtype_io", i32), ("dtype_bc", i32),
                ("dt_softplus", i32),
                ("x_bs", i64), ("dt_bs", i64), ("z_bs", i64), ("out_bs", i64), ("B_bs", i64), ("C_bs", i64),
                ("state", vp), ("x", vp), ("dt", vp), ("A", vp), ("Bm", vp), ("Cm", vp), ("D", vp), ("z", vp),
                ("dt_bias", vp), ("out", vp), ("dt_rank", i32), ("dt_w", vp), ("out_packed", vp)]


class RowsArgs(C.Structure):
    _fields_ = [("M", i32), ("N", i32), ("K", i32), ("act", i32), ("ldx", i64), ("ldw", i64), ("ldy", i64),
                ("x", vp), ("W", vp), ("bias", vp), ("y", vp),
                ("conv_dim", i32), ("conv_state", vp), ("conv_w", vp), ("conv_b", vp), ("u", vp), ("ldu", i64),
                ("ln_w", vp), ("ln_b", vp), ("ln_eps", f32), ("gamma", vp), ("beta", vp), ("ld_gb", i64),
                ("res", vp), ("ld_res", i64), ("kgroups", i32), ("splitk_slab", vp), ("splitk_count", vp),
                ("w_packed", i32), ("x_packed", i32), ("y_packed", vp), ("u_packed", vp)]


class CrossEntropyArgs(C.Structure):
    _fields_ = [("rows", i64), ("vocab", i32), ("dtype", i32), ("ld", i64), ("logits", vp), ("targets", vp),
                ("ignore_index", i32), ("loss", vp), ("lse", vp), ("workspace", vp)]


class GemmArgs(C.Structure):
    _fields_ = [("m", i32), ("n", i32), ("k", i32), ("layout", i32), ("splits", i32), ("epilogue", i32),
                ("out_dtype", i32), ("bias_dtype", i32), ("lda", i64), ("ldb", i64), ("ldc", i64), ("ld_aux", i64),
                ("a", vp), ("b", vp), ("c", vp), ("bias", vp), ("aux", vp), ("workspace", vp), ("beta", f32)]


class DropoutArgs(C.Structure):
    _fields_ = [("n", i64), ("dtype", i32), ("p", f32), ("seed", C.c_uint64), ("x", vp), ("y", vp), ("pre", vp),
                ("group", i32), ("x_rep", i32), ("x_inner", i32), ("reserved_", i32), ("seed_in", vp),
                ("seed_out", vp)]


class SampleArgs(C.Structure):
    _fields_ = [("rows", i32), ("vocab", i32), ("dtype", i32), ("top_k", i32), ("ld", i64), ("logits", vp),
                ("bias", vp), ("bias_ld", i64), ("temperature", f32), ("top_p", f32), ("seed", vp), ("step", vp),
                ("advance", i32), ("step0", i32), ("pos", vp), ("tokens", vp), ("tok_stride", i64),
                ("history", vp), ("hist_ld", i64), ("hist_cols", i32), ("eos_id", i32), ("pad_id", i32),
                ("pos_rows", i32), ("finished", vp), ("length", vp), ("unfinished", vp)]


class SampleRowsArgs(C.Structure):
    _fields_ = [("rows", i32), ("vocab", i32), ("dtype", i32), ("window", i32), ("ld", i64), ("logits", vp),
                ("bias", vp), ("bias_ld", i64), ("temperature", vp), ("top_k", vp), ("top_p", vp), ("seed", vp),
                ("draw", vp), ("penalty", vp), ("max_length", vp), ("step", vp), ("advance", i32), ("step0", i32),
                ("pos", vp), ("tokens", vp), ("tok_stride", i64), ("history", vp), ("hist_ld", i64),
                ("hist_cols", i32), ("eos_id", i32), ("pad_id", i32), ("pos_rows", i32), ("finished", vp),
                ("length", vp), ("unfinished", vp)]


class SampleLogprobOut(C.Structure):
    _fields_ = [("logprob", vp), ("logprob_history", vp), ("lp_ld", i64)]


class RowMap(C.Structure):
    _fields_ = [("ptr", vp), ("seg_rows", i64), ("seg_stride", i64), ("row_stride", i64), ("halo_c", i32),
                ("halo_p", i32)]


class ConvGemmArgs(C.Structure):
    _fields_ = [("layout", i32), ("m", i32), ("n", i32), ("k", i32), ("a", RowMap), ("b", RowMap), ("c", RowMap),
                ("aux", RowMap), ("bias", vp), ("epilogue", i32), ("beta", f32), ("splits", i32),
                ("workspace", vp), ("colsum_a", vp)]


class SkinnyArgs(C.Structure):
    _fields_ = [("mode", i32), ("m", i32), ("n", i32), ("k", i32), ("c_dtype", i32), ("beta", f32),
                ("lda", i64), ("ldb", i64), ("ldc", i64), ("a", vp), ("b", vp), ("c", vp), ("workspace", vp),
                ("trans_c", i32), ("reserved_", i32)]


class LNArgs(C.Structure):
    _fields_ = [("rows", i32), ("cols", i32), ("dtype", i32), ("rows_per_group", i32), ("eps", f32),
                ("x_rs", i64), ("res_rs", i64), ("xsum_rs", i64), ("y_rs", i64), ("gb_rs", i64),
                ("x", vp), ("res", vp), ("x_sum", vp), ("w", vp), ("b", vp), ("gamma", vp), ("beta", vp),
                ("gb_dtype", i32), ("y", vp), ("mean", vp), ("rstd", vp)]


class LNBwdArgs(C.Structure):
    _fields_ = [("f", LNArgs), ("dy", vp), ("dy_rs", i64), ("dx_acc", vp), ("dxacc_rs", i64),
                ("dx", vp), ("dx_rs", i64), ("dw", vp), ("db", vp), ("dgamma", vp), ("dbeta", vp),
                ("workspace", vp), ("dx_colsum", vp), ("dgb_rs", i64)]


class AttnFwdArgs(C.Structure):
    _fields_ = [("batch", i32), ("heads", i32), ("head_dim", i32), ("q_len", i32), ("kv_len", i32),
                ("dtype", i32), ("scale", f32),
                ("q_bs", i64), ("q_ls", i64), ("k_bs", i64), ("k_ls", i64), ("v_bs", i64), ("v_ls", i64),
                ("o_bs", i64), ("o_ls", i64), ("mask_bs", i64),
                ("q", vp), ("k", vp), ("v", vp), ("key_padding_mask", vp), ("out", vp), ("lse", vp),
                ("out_packed", vp), ("kv_hs", i64)]


class AttnQProjArgs(C.Structure):
    _fields_ = [("f", AttnFwdArgs), ("x", vp), ("x_rs", i64), ("wq", vp), ("bq", vp), ("ln_w", vp), ("ln_b", vp),
                ("eps", f32), ("d_model", i32)]


class AttnDecodeSplitArgs(C.Structure):
    _fields_ = [("f", AttnFwdArgs), ("kv_lens", vp), ("workspace", vp), ("workspace_bytes", i64)]


class AttnDecodeSplitSharedArgs(C.Structure):
    _fields_ = [("s", AttnDecodeSplitArgs), ("kv_rows", vp), ("kv_batch", i32)]


class KvQuantizeFp8Args(C.Structure):
    _fields_ = [("rows", i32), ("heads", i32), ("head_dim", i32), ("kv_len", i32), ("dtype", i32), ("reserved_", i32),
                ("x_bs", i64), ("x_ls", i64), ("out_bs", i64), ("scale_bs", i64),
                ("x", vp), ("kv_lens", vp), ("out", vp), ("scale", vp), ("workspace", vp), ("workspace_bytes", i64)]


class AttnDecodeSplitFp8Args(C.Structure):
    _fields_ = [("s", AttnDecodeSplitArgs), ("k_scale", vp), ("v_scale", vp), ("scale_bs", i64)]


class AttnBwdArgs(C.Structure):
    _fields_ = [("f", AttnFwdArgs), ("dout", vp), ("do_bs", i64), ("do_ls", i64),
                ("dq", vp), ("dq_bs", i64), ("dq_ls", i64), ("dk", vp), ("dk_bs", i64), ("dk_ls", i64),
                ("dv", vp), ("dv_bs", i64), ("dv_ls", i64), ("workspace", vp)]


class CastDesc(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("dstT", vp), ("rows", i32), ("cols", i32), ("tile0", i64)]


class AdamTensor(C.Structure):
    _fields_ = [("p", vp), ("g", vp), ("m", vp), ("v", vp), ("n", i64), ("chunk0", i64)]


ADAMW_MAX_GROUPS = 64
# offsets into mtts_clip_adamw's `out` (include/mtts.h MTTS_ADAMW_OUT_*)
ADAMW_OUT_LR, ADAMW_OUT_STEP, ADAMW_OUT_BC2, ADAMW_OUT_DECAY, ADAMW_OUT_FLOATS = 8, 72, 136, 200, 264
LR_KINDS = {"constant": 0, "cosine": 1, "linear": 2, "inverse_sqrt": 3}


class AdamWTensor(C.Structure):
    _fields_ = [("p", vp), ("g", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("ema", vp), ("n", i64), ("chunk0", i64),
                ("group", i32), ("reserved_", i32)]


class AdamWGroup(C.Structure):
    _fields_ = [("lr", f32), ("weight_decay", f32), ("decoupled", i32), ("clip", i32)]


class LrSchedule(C.Structure):
    _fields_ = [("kind", i32), ("warmup_steps", i32), ("total_steps", i32), ("reserved_", i32),
                ("min_ratio", C.c_double)]


class AdamWArgs(C.Structure):
    _fields_ = [("beta1", f32), ("beta2", f32), ("eps", f32), ("max_norm", f32), ("ngroups", i32),
                ("ema_warmup", i32), ("skip_nonfinite", i32), ("reserved_", i32), ("ema_decay", C.c_double),
                ("active_groups", C.c_uint64), ("total_chunks", i64), ("clip_chunks", i64), ("schedule", LrSchedule)]


MDN_MAX_K = 32
MDN_MODES = {"isotropic_across_clusters": 0, "isotropic": 1, "diagonal": 2, "fixed": 3}
MDN_NOISE_NONE, MDN_NOISE_GIVEN, MDN_NOISE_DRAWN = 0, 1, 2


class MdnParamsArgs(C.Structure):
    _fields_ = [("rows", i32), ("K", i32), ("d", i32), ("mode", i32), ("dtype", i32), ("noise", i32),
                ("logits_rs", i64), ("pi_rs", i64), ("sraw_rs", i64), ("sigma_rs", i64), ("eps_rs", i64),
                ("pi_logits", vp), ("sigma_raw", vp), ("eps", vp), ("noise_scale", vp), ("row_seed", vp),
                ("seed_in", vp), ("seed_out", vp), ("pi", vp), ("sigma", vp)]


class MdnParamsBwdArgs(C.Structure):
    _fields_ = [("f", MdnParamsArgs), ("dpi", vp), ("dpi_rs", i64), ("dsigma", vp), ("dsigma_rs", i64),
                ("dlogits", vp), ("dlogits_rs", i64), ("dsigma_raw", vp), ("dsraw_rs", i64),
                ("dnoise_scale", vp), ("workspace", vp)]


class MixtureNllArgs(C.Structure):
    _fields_ = [("rows", i32), ("K", i32), ("d", i32), ("mode", i32), ("dtype", i32), ("reserved_", i32),
                ("y_rs", i64), ("pi_rs", i64), ("mu_rs", i64), ("sigma_rs", i64),
                ("y", vp), ("pi", vp), ("mu", vp), ("sigma", vp), ("loss", vp), ("lse", vp)]


class MixtureNllBwdArgs(C.Structure):
    _fields_ = [("f", MixtureNllArgs), ("grad_loss", vp), ("dy", vp), ("dy_rs", i64), ("dpi", vp), ("dpi_rs", i64),
                ("dmu", vp), ("dmu_rs", i64), ("dsigma", vp), ("dsigma_rs", i64)]


class MixtureSampleArgs(C.Structure):
    _fields_ = [("rows", i32), ("K", i32), ("d", i32), ("mode", i32), ("dtype", i32), ("reserved_", i32),
                ("pi_rs", i64), ("mu_rs", i64), ("sigma_rs", i64), ("out_rs", i64),
                ("pi", vp), ("mu", vp), ("sigma", vp), ("seed", vp), ("draw", vp), ("seed_in", vp),
                ("out", vp), ("component", vp)]


class ReluDropoutArgs(C.Structure):
    _fields_ = [("n", i64), ("dtype", i32), ("p", f32), ("seed", C.c_uint64), ("x", vp), ("y_fwd", vp), ("out", vp),
                ("seed_in", vp), ("seed_out", vp)]


class RowLNArgs(C.Structure):
    _fields_ = [("rows", i32), ("cols", i32), ("dtype", i32), ("eps", f32), ("x_rs", i64), ("y_rs", i64),
                ("x", vp), ("w", vp), ("b", vp), ("y", vp), ("mean", vp), ("rstd", vp)]


class RowLNBwdArgs(C.Structure):
    _fields_ = [("f", RowLNArgs), ("dy", vp), ("dy_rs", i64), ("dx", vp), ("dx_rs", i64), ("dw", vp), ("db", vp)]


_SIGS = {
    "mtts_abi_version": ([], i32),
    "mtts_last_error": ([], C.c_char_p),
    "mtts_set_override": ([i32, i32], i32),
    "mtts_get_override": ([i32], i32),
    "mtts_selective_scan_fwd_workspace": ([i32, i32, i32, i32], i64),
    "mtts_selective_scan_fwd": ([C.POINTER(ScanFwdArgs), vp], i32),
    "mtts_selective_scan_bwd_workspace": ([i32, i32, i32, i32], i64),
    "mtts_selective_scan_bwd": ([C.POINTER(ScanBwdArgs), vp], i32),
    "mtts_causal_conv1d_fwd": ([C.POINTER(ConvFwdArgs), vp], i32),
    "mtts_causal_conv1d_bwd_workspace": ([i32, i32, i32, i32], i64),
    "mtts_causal_conv1d_bwd": ([C.POINTER(ConvBwdArgs), vp], i32),
    "mtts_causal_conv1d_update": ([C.POINTER(ConvUpdateArgs), vp], i32),
    "mtts_selective_state_update": ([C.POINTER(StateUpdateArgs), vp], i32),
    "mtts_layernorm_fwd": ([C.POINTER(LNArgs), vp], i32),
    "mtts_gemm_rows": ([C.POINTER(RowsArgs), vp], i32),
    "mtts_pack_rows_bytes": ([i32, i32], i64),
    "mtts_cross_entropy_workspace": ([i64], i64),
    "mtts_cross_entropy_fwd": ([C.POINTER(CrossEntropyArgs), vp], i32),
    "mtts_cross_entropy_bwd": ([C.POINTER(CrossEntropyArgs), vp, vp, i64, vp], i32),
    "mtts_layernorm_rows_packed": ([C.POINTER(LNArgs), vp, vp], i32),
    "mtts_pack_rows_weight": ([vp, i64, i32, i32, vp, vp], i32),
    "mtts_gemm_workspace": ([C.POINTER(GemmArgs)], i64),
    "mtts_gemm": ([C.POINTER(GemmArgs), vp], i32),
    "mtts_gemm_grouped": ([C.POINTER(GemmArgs), i32, vp], i32),
    "mtts_gemm_grouped_rounds": ([C.POINTER(GemmArgs), i32, vp], i32),
    "mtts_convgemm": ([C.POINTER(ConvGemmArgs), vp], i32),
    "mtts_convgemm_workspace": ([C.POINTER(ConvGemmArgs)], i64),
    "mtts_gemm_skinny": ([C.POINTER(SkinnyArgs), vp], i32),
    "mtts_gemm_skinny_workspace": ([C.POINTER(SkinnyArgs)], i64),
    "mtts_layernorm_bwd_workspace": ([i32, i32, i32], i64),
    "mtts_layernorm_bwd": ([C.POINTER(LNBwdArgs), vp], i32),
    "mtts_colsum_workspace": ([i32, i32, i32], i64),
    "mtts_colsum": ([vp, i32, i32, i32, i64, i32, vp, i64, vp, vp], i32),
    "mtts_attention_fwd": ([C.POINTER(AttnFwdArgs), vp], i32),
    "mtts_attention_decode_qproj": ([C.POINTER(AttnQProjArgs), vp], i32),
    "mtts_attention_decode_split_workspace": ([i32, i32, i32, i32], i64),
    "mtts_attention_decode_split": ([C.POINTER(AttnDecodeSplitArgs), vp], i32),
    "mtts_attention_decode_split_shared": ([C.POINTER(AttnDecodeSplitSharedArgs), vp], i32),
    "mtts_attention_decode_split_fp8": ([C.POINTER(AttnDecodeSplitFp8Args), vp], i32),
    "mtts_kv_quantize_fp8_workspace": ([i32, i32, i32, i32], i64),
    "mtts_kv_quantize_fp8": ([C.POINTER(KvQuantizeFp8Args), vp], i32),
    "mtts_attention_bwd_workspace": ([i32, i32, i32, i32, i32, i32], i64),
    "mtts_attention_bwd": ([C.POINTER(AttnBwdArgs), vp], i32),
    "mtts_adam_chunks": ([i64], i64),
    "mtts_adam_workspace": ([i64], i64),
    "mtts_clip_adam": ([vp, i32, i64, vp, f32, f32, f32, f32, f32, f32, vp, vp, vp], i32),
    "mtts_clip_adamw": ([vp, i32, vp, C.POINTER(AdamWArgs), vp, vp, vp, vp, vp], i32),
    "mtts_embed_sum": ([vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i64, vp, vp], i32),
    "mtts_embed_sum_at": ([vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i64, vp, i64, i32, vp], i32),
    "mtts_embed_table_grad_workspace": ([i64, i32, i32], i64),
    "mtts_embed_table_grad": ([vp, i64, vp, i32, i64, i32, i32, vp, vp, vp], i32),
    "mtts_cast_tiles": ([i32, i32], i64),
    "mtts_cast_bf16_multi": ([vp, i32, i64, vp], i32),
    "mtts_length_regulate_lengths": ([vp, i64, i32, i32, vp, vp], i32),
    "mtts_length_regulate_fwd": ([vp, i32, i32, i32, i32, i64, i64, vp, i64, i32, vp, i64, i64, vp], i32),
    "mtts_length_regulate_bwd": ([vp, i32, i32, i32, i32, i64, i64, vp, i64, i32, vp, i64, i64, vp], i32),
    "mtts_dropout": ([C.POINTER(DropoutArgs), vp], i32),
    "mtts_sample_tokens": ([C.POINTER(SampleArgs), vp], i32),
    "mtts_sample_tokens_rows": ([C.POINTER(SampleRowsArgs), vp], i32),
    "mtts_sample_tokens_slots": ([C.POINTER(SampleRowsArgs), vp], i32),
    "mtts_sample_tokens_lp": ([C.POINTER(SampleArgs), C.POINTER(SampleLogprobOut), vp], i32),
    "mtts_sample_tokens_rows_lp": ([C.POINTER(SampleRowsArgs), C.POINTER(SampleLogprobOut), vp], i32),
    "mtts_sample_tokens_slots_lp": ([C.POINTER(SampleRowsArgs), C.POINTER(SampleLogprobOut), vp], i32),
    "mtts_mdn_params_fwd": ([C.POINTER(MdnParamsArgs), vp], i32),
    "mtts_mdn_params_bwd": ([C.POINTER(MdnParamsBwdArgs), vp], i32),
    "mtts_mixture_nll_fwd": ([C.POINTER(MixtureNllArgs), vp], i32),
    "mtts_mixture_nll_bwd": ([C.POINTER(MixtureNllBwdArgs), vp], i32),
    "mtts_mixture_sample": ([C.POINTER(MixtureSampleArgs), vp], i32),
    "mtts_relu_dropout": ([C.POINTER(ReluDropoutArgs), vp], i32),
    "mtts_mdn_layernorm_fwd": ([C.POINTER(RowLNArgs), vp], i32),
    "mtts_mdn_layernorm_bwd": ([C.POINTER(RowLNBwdArgs), vp], i32),
}

_lib = None


def lib():
    """Load libmtts.so once (raises if it is missing or ABI-incompatible)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libmtts.so not found at {LIB_PATH}; run __graft_entry__.build() "
                               "(make -C mamba-tts-project_amd/mtts/csrc)")
        L = C.CDLL(LIB_PATH)
        # ABI 15 grew by additions only, so a library built before them reports
        # the same version: the added symbols tell them apart
        for sym, what in (("mtts_embed_sum_at", "ragged prompts"),
                          ("mtts_sample_tokens_rows", "per-row sampling"),
                          ("mtts_sample_tokens_slots", "decode sessions"),
                          ("mtts_gemm_grouped_rounds", "round-filling weight gradients"),
                          ("mtts_attention_decode_split", "long-conditioning decode"),
                          ("mtts_sample_tokens_slots_lp", "token log-probabilities"),
                          ("mtts_attention_decode_split_shared", "shared-key samples"),
                          ("mtts_attention_decode_split_fp8", "FP8 conditioning K/V"),
                          ("mtts_clip_adamw", "grouped AdamW step"),
                          ("mtts_mixture_sample", "SMSD mixture-density head")):
            if not hasattr(L, sym):
                raise RuntimeError(f"{LIB_PATH} is stale: it was built before {sym} ({what}) was "
                                   "added; rebuild it with __graft_entry__.build() "
                                   "(make -C mamba-tts-project_amd/mtts/csrc)")
        for name, (argt, rest) in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = rest
        v = L.mtts_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"libmtts ABI {v} != expected {ABI_VERSION}")
        _lib = L
    return _lib


def exported_symbols():
    return list(_SIGS)


def call(name, args, *more):
    """Invoke ``name(&args, [&more...,] current_stream)``; raise on error."""
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    rc = getattr(L, name)(C.byref(args), *[C.byref(m) for m in more], C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {L.mtts_last_error().decode()}")


def call_raw(name, *args):
    """Invoke a non-struct entry point; the current stream is appended."""
    L = lib()
    rc = getattr(L, name)(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {L.mtts_last_error().decode()}")


# kernel-path override keys (include/mtts.h MTTS_OVR_*): test / measurement hooks
OVERRIDES = {"scan_path": 0, "scan_p": 1, "scan_segs": 2, "scan_bwd_segs": 3, "gemm_narrow": 4,
             "attn_chunks": 5, "attn_bwd": 6, "attn_generic": 7, "conv_untiled": 8, "gemm_tile": 9,
             "attn_dq_dma": 10}
SCAN_C1, SCAN_W2, SCAN_NARROW = 1, 2, 3
ATTN_BWD_FUSED, ATTN_BWD_SPLIT = 1, 2


@contextlib.contextmanager
def override(**paths):
    """Force kernel paths for the duration of the block (mtts_set_override),
    e.g. ``with override(scan_path=SCAN_W2, scan_segs=3): ...``; None leaves a
    key automatic.  The previous values are restored on exit."""
    L = lib()
    old = {}
    try:
        for k, v in paths.items():
            old[k] = L.mtts_set_override(OVERRIDES[k], -1 if v is None else int(v))
        yield
    finally:
        for k, v in old.items():
            L.mtts_set_override(OVERRIDES[k], v)


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype} (libmtts takes float32 / bfloat16)")


def ptr(t):
    return None if t is None else t.data_ptr()
