"""The SMSD mixture-density head's arithmetic on libmtts (csrc/mdn.hip).

Reference smsd.py: MDNHead.forward's softmax / NoiseNet / softplus (:239-264,
:277-292), mixture_nll_loss (:295-372), SMSD.sample (:127-164) and the MLP's
ReLU -> Dropout pairs (:192-196).  Each is one HIP launch (the loss and the
noise-scale gradient add a one-workgroup sum), fp32 math on fp32 / bf16
tensors, deterministic; no CPU path.

Random draws are counter-based (include/mtts.h, "SMSD mixture-density head"):
a row's values are a function of its seed, its draw count and the element
index, plus the per-device base of mtts.dropout that `dropout.advance()` moves,
so a step replayed from a hipGraph draws fresh values.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import dropout as D

MODES = L.MDN_MODES
ROW_SEED_STEP = 0x2545F4914F6CDD1D     # odd: the rows of one integer seed get distinct streams


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libmtts ops need CUDA (HIP) tensors; there is no CPU path")


def mode_code(variance_mode: str) -> int:
    if variance_mode not in MODES:
        raise ValueError(f"unknown variance_mode {variance_mode!r} (one of {sorted(MODES)})")
    return MODES[variance_mode]


def sigma_len(mode: int, K: int, d: int) -> int:
    return (1, K, K * d, 0)[mode]


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def row_seeds(seed, rows: int, device) -> torch.Tensor:
    """(rows,) int64 device seeds: a tensor is taken as it is (one seed per
    row); an int s gives row r the seed s + r * ROW_SEED_STEP (mod 2^64);
    None draws s from torch's CPU generator (mtts.dropout.new_seed)."""
    if isinstance(seed, torch.Tensor):
        if seed.shape != (rows,) or seed.dtype != torch.int64:
            raise ValueError(f"seed tensor must be ({rows},) int64, got {tuple(seed.shape)} {seed.dtype}")
        _need_cuda(seed)
        return seed.contiguous()
    s = D.new_seed() if seed is None else int(seed)
    return torch.arange(rows, device=device, dtype=torch.int64) * ROW_SEED_STEP + _wrap64(s)


def _rows2(t, rows):
    """(rows, n) contiguous view of a per-row tensor."""
    return t.reshape(rows, -1).contiguous()


# --------------------------------------------------------------------- ReLU + dropout

def _relu_dropout_call(x, y_fwd, p, seed, seed_in, seed_out):
    out = torch.empty_like(x)
    a = L.ReluDropoutArgs()
    a.n, a.dtype, a.p, a.seed = x.numel(), L.dtype_code(x), float(p), seed & (2 ** 64 - 1)
    a.x, a.y_fwd, a.out = x.data_ptr(), L.ptr(y_fwd), out.data_ptr()
    a.seed_in, a.seed_out = L.ptr(seed_in), L.ptr(seed_out)
    L.call("mtts_relu_dropout", a)
    return out


class ReluDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        _need_cuda(x)
        ctx.p = p
        x = x.contiguous()
        base = used = None
        if p > 0.0:
            seed = D.new_seed() if seed is None else seed
            base, used = D.device_base(x.device), torch.empty(1, dtype=torch.int64, device=x.device)
        y = _relu_dropout_call(x, None, p, seed or 0, base, used)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _relu_dropout_call(dy.contiguous().to(y.dtype), y, ctx.p, 0, None, None), None, None


def relu_dropout(x: torch.Tensor, p: float, training: bool, seed: int = None) -> torch.Tensor:
    """F.dropout(F.relu(x), p, training) in one HIP pass; a plain ReLU when
    not training or p == 0.  The mask is mtts.dropout's (same hash, same seed
    plumbing); the backward masks by y > 0 and reads no seed."""
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
    return ReluDropoutFn.apply(x, p, seed)


# --------------------------------------------------------------------- LayerNorm, any width

def _rowln_args(x2, w, b, eps, y, mean, rstd):
    a = L.RowLNArgs()
    a.rows, a.cols, a.dtype, a.eps = x2.shape[0], x2.shape[1], L.dtype_code(x2), float(eps)
    a.x, a.x_rs, a.y, a.y_rs = x2.data_ptr(), x2.stride(0), y.data_ptr(), y.stride(0)
    a.w, a.b, a.mean, a.rstd = w.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    return a


class RowLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        _need_cuda(x, w, b)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        wf, bf = w.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()
        y = torch.empty_like(x2)
        mean = torch.empty(x2.shape[0], device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        L.call("mtts_mdn_layernorm_fwd", _rowln_args(x2, wf, bf, eps, y, mean, rstd))
        ctx.save_for_backward(x2, wf, bf, y, mean, rstd)
        ctx.eps, ctx.meta = eps, (x.shape, w.dtype, b.dtype)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, wf, bf, y, mean, rstd = ctx.saved_tensors
        g = L.RowLNBwdArgs()
        g.f = _rowln_args(x2, wf, bf, ctx.eps, y, mean, rstd)
        dy2 = dy.reshape(x2.shape).to(x2.dtype).contiguous()
        dx = torch.empty_like(x2)
        dw, db = torch.empty_like(wf), torch.empty_like(bf)
        g.dy, g.dy_rs, g.dx, g.dx_rs, g.dw, g.db = dy2.data_ptr(), dy2.stride(0), dx.data_ptr(), dx.stride(0), dw.data_ptr(), db.data_ptr()
        L.call("mtts_mdn_layernorm_bwd", g)
        shape, wd, bd = ctx.meta
        return dx.view(shape), dw.to(wd), db.to(bd), None


def layer_norm_rows(x, w, b, eps=1e-5):
    """F.layer_norm over the last dimension at ANY width (csrc/mdn.hip): the
    head's input LayerNorm where ops.layer_norm's kernels do not apply (widths
    that are not a multiple of 64)."""
    return RowLayerNormFn.apply(x, w, b, eps)


# --------------------------------------------------------------------- parameters

class MdnParamsFn(torch.autograd.Function):
    """(pi, sigma_flat) from (pi_logits (B, K), sigma_raw (B, S) | None)."""

    @staticmethod
    def forward(ctx, pi_logits, sigma_raw, noise_scale, eps, seeds, mode, K, d):
        _need_cuda(pi_logits, sigma_raw, eps)
        B = pi_logits.shape[0]
        dt = pi_logits.dtype
        lg = _rows2(pi_logits, B)
        S = sigma_len(mode, K, d)
        a = L.MdnParamsArgs()
        a.rows, a.K, a.d, a.mode, a.dtype = B, K, d, mode, L.dtype_code(lg)
        pi = torch.empty(B, K, device=lg.device, dtype=dt)
        a.pi_logits, a.logits_rs, a.pi, a.pi_rs = lg.data_ptr(), lg.stride(0), pi.data_ptr(), K
        keep = [lg, pi]
        sigma = used = None
        a.noise = L.MDN_NOISE_NONE
        if S:
            sr = _rows2(sigma_raw.to(dt), B)
            if sr.shape[1] != S:
                raise ValueError(f"sigma_raw has {sr.shape[1]} elements per row, the mode needs {S}")
            sigma = torch.empty(B, S, device=lg.device, dtype=dt)
            a.sigma_raw, a.sraw_rs, a.sigma, a.sigma_rs = sr.data_ptr(), S, sigma.data_ptr(), S
            keep += [sr, sigma]
            if eps is not None:
                e = _rows2(eps.to(dt), B)
                if e.shape[1] != S:
                    raise ValueError("epsilon must have sigma_raw's shape")
                a.noise, a.eps, a.eps_rs = L.MDN_NOISE_GIVEN, e.data_ptr(), S
                keep.append(e)
            elif seeds is not None:
                used = torch.empty(1, dtype=torch.int64, device=lg.device)
                a.noise, a.row_seed = L.MDN_NOISE_DRAWN, seeds.data_ptr()
                a.seed_in, a.seed_out = D.device_base(lg.device).data_ptr(), used.data_ptr()
                keep += [seeds, used]
            if a.noise != L.MDN_NOISE_NONE:
                ns = noise_scale.detach().to(torch.float32).reshape(1)
                a.noise_scale = ns.data_ptr()
                keep.append(ns)
        L.call("mtts_mdn_params_fwd", a)
        if used is not None:
            a.seed_in, a.seed_out = used.data_ptr(), None     # the backward reads the recorded base
        ctx.args, ctx.keep, ctx.S = a, keep, S
        ctx.ns_meta = None if noise_scale is None else (noise_scale.shape, noise_scale.dtype)
        ctx.sraw_meta = None if sigma_raw is None else (sigma_raw.shape, sigma_raw.dtype)
        ctx.lg_shape = pi_logits.shape
        if sigma is None:
            sigma = pi.new_empty(0)
            ctx.mark_non_differentiable(sigma)
        return pi, sigma

    @staticmethod
    def backward(ctx, dpi, dsigma):
        a, S = ctx.args, ctx.S
        B, K = a.rows, a.K
        dev, dt = dpi.device, ctx.keep[0].dtype
        g = L.MdnParamsBwdArgs()
        g.f = a
        dpi = dpi.to(dt).contiguous()
        dlog = torch.empty(B, K, device=dev, dtype=dt)
        g.dpi, g.dpi_rs, g.dlogits, g.dlogits_rs = dpi.data_ptr(), K, dlog.data_ptr(), K
        dsraw = dns = None
        if S:
            dsg = dsigma.to(dt).contiguous()
            dsraw = torch.empty(B, S, device=dev, dtype=dt)
            ws = torch.empty(B, device=dev, dtype=torch.float32)
            g.dsigma, g.dsigma_rs, g.dsigma_raw, g.dsraw_rs, g.workspace = dsg.data_ptr(), S, dsraw.data_ptr(), S, ws.data_ptr()
            if a.noise != L.MDN_NOISE_NONE:
                dns = torch.empty(1, device=dev, dtype=torch.float32)
                g.dnoise_scale = dns.data_ptr()
        L.call("mtts_mdn_params_bwd", g)
        if dsraw is not None:
            dsraw = dsraw.view(ctx.sraw_meta[0]).to(ctx.sraw_meta[1])
        if dns is not None:
            dns = dns.view(ctx.ns_meta[0]).to(ctx.ns_meta[1])
        return dlog.view(ctx.lg_shape), dsraw, dns, None, None, None, None, None


def mdn_params(pi_logits, sigma_raw, noise_scale, variance_mode, style_dim, training=False, epsilon=None, seed=None):
    """(pi (B, K), sigma) of MDNHead.forward from the heads' raw outputs:
    softmax, and softplus(sigma_raw [+ noise_scale * eps in training]).  sigma
    has the reference's shape for the mode ((B,), (B, K), (B, K, d); 0.1 *
    ones(B) for "fixed").  `epsilon`: the NoiseNet noise, sigma_raw's shape;
    otherwise it is drawn in the kernel from `seed` (see `row_seeds`)."""
    mode = mode_code(variance_mode)
    B, K = pi_logits.shape
    _need_cuda(pi_logits)
    if mode == MODES["fixed"]:
        pi, _ = MdnParamsFn.apply(pi_logits, None, None, None, None, mode, K, style_dim)
        return pi, torch.full((B,), 0.1, device=pi_logits.device, dtype=pi_logits.dtype)
    seeds = None
    if training and epsilon is None:
        seeds = row_seeds(seed, B, pi_logits.device)
    pi, sg = MdnParamsFn.apply(pi_logits, sigma_raw, noise_scale if training else None,
                               epsilon if training else None, seeds, mode, K, style_dim)
    if mode == MODES["isotropic_across_clusters"]:
        return pi, sg.view(B)
    if mode == MODES["isotropic"]:
        return pi, sg.view(B, K)
    return pi, sg.view(B, K, style_dim)


# --------------------------------------------------------------------- loss

def _nll_args(y, pi, mu, sigma, mode, loss, lse):
    B, K, d = mu.shape
    a = L.MixtureNllArgs()
    a.rows, a.K, a.d, a.mode, a.dtype = B, K, d, mode, L.dtype_code(mu)
    a.y, a.y_rs, a.pi, a.pi_rs, a.mu, a.mu_rs = y.data_ptr(), d, pi.data_ptr(), K, mu.data_ptr(), K * d
    if sigma is not None:
        a.sigma, a.sigma_rs = sigma.data_ptr(), sigma_len(mode, K, d)
    a.loss, a.lse = loss.data_ptr(), lse.data_ptr()
    return a


def _check_mixture(pi, mu, sigma, mode):
    _need_cuda(pi, mu, sigma)
    if mu.dim() != 3 or pi.shape != mu.shape[:2]:
        raise ValueError(f"mixture: pi {tuple(pi.shape)} / mu {tuple(mu.shape)} must be (B, K) / (B, K, d)")
    B, K, d = mu.shape
    if not 1 <= K <= L.MDN_MAX_K:
        raise ValueError(f"mixture: K={K} must be in [1, {L.MDN_MAX_K}]")
    if mu.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"unsupported dtype {mu.dtype} (libmtts takes float32 / bfloat16)")
    want = ((B,), (B, K), (B, K, d), None)[mode]
    if want is not None and tuple(sigma.shape) != want:
        raise ValueError(f"mixture: sigma {tuple(sigma.shape)} must be {want} in this variance mode")


class MixtureNllFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, pi, mu, sigma, mode):
        _check_mixture(pi, mu, sigma, mode)
        B, K, d = mu.shape
        if y.shape != (B, d):
            raise ValueError(f"mixture_nll_loss: y_true {tuple(y.shape)} must be ({B}, {d})")
        dt = mu.dtype
        fixed = mode == MODES["fixed"]
        yc, pc, mc = y.to(dt).contiguous(), pi.to(dt).contiguous(), mu.contiguous()
        sc = None if fixed else sigma.to(dt).contiguous()
        loss = torch.empty(1, device=mu.device, dtype=torch.float32)
        lse = torch.empty(B, device=mu.device, dtype=torch.float32)
        L.call("mtts_mixture_nll_fwd", _nll_args(yc, pc, mc, sc, mode, loss, lse))
        ctx.save_for_backward(yc, pc, mc, sc, loss, lse)
        ctx.mode = mode
        ctx.meta = (y.dtype, pi.dtype, None if sigma is None else (sigma.shape, sigma.dtype))
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        yc, pc, mc, sc, loss, lse = ctx.saved_tensors
        g = L.MixtureNllBwdArgs()
        g.f = _nll_args(yc, pc, mc, sc, ctx.mode, loss, lse)
        B, K, d = mc.shape
        gl = gl.reshape(1).to(torch.float32).contiguous()
        dy, dpi, dmu = torch.empty_like(yc), torch.empty_like(pc), torch.empty_like(mc)
        dsg = None if sc is None else torch.empty_like(sc)
        g.grad_loss, g.dy, g.dy_rs, g.dpi, g.dpi_rs, g.dmu, g.dmu_rs = gl.data_ptr(), dy.data_ptr(), d, dpi.data_ptr(), K, dmu.data_ptr(), K * d
        if dsg is not None:
            g.dsigma, g.dsigma_rs = dsg.data_ptr(), sigma_len(ctx.mode, K, d)
        L.call("mtts_mixture_nll_bwd", g)
        ydt, pdt, smeta = ctx.meta
        if dsg is not None:
            dsg = dsg.view(smeta[0]).to(smeta[1])
        return dy.to(ydt), dpi.to(pdt), dmu, dsg, None


def mixture_nll(y_true, pi, mu, sigma, variance_mode="isotropic_across_clusters"):
    """smsd.py's mixture_nll_loss on the HIP kernel (fp32 scalar); in the
    default mode row b's variance serves every component of row b."""
    return MixtureNllFn.apply(y_true, pi, mu, sigma, mode_code(variance_mode))


# --------------------------------------------------------------------- sampler

@torch.no_grad()
def mixture_sample(pi, mu, sigma, variance_mode, seed=None, draw=None, return_component=False, use_base=True):
    """One style vector per row, (B, d) in mu's dtype, without gradient:
    component by inverse CDF over pi, then mu_k + std * z.  `seed`: int or
    (B,) int64 tensor (see `row_seeds`); `draw`: optional (B,) int64 draw
    counts; `use_base`: add mtts.dropout's per-device base (moved by
    dropout.advance())."""
    mode = mode_code(variance_mode)
    pi, mu = pi.detach(), mu.detach()
    sigma = None if (sigma is None or mode == MODES["fixed"]) else sigma.detach()
    _check_mixture(pi, mu, sigma, mode)
    B, K, d = mu.shape
    dt = mu.dtype
    pc, mc = pi.to(dt).contiguous(), mu.contiguous()
    sc = None if sigma is None else sigma.to(dt).contiguous()
    seeds = row_seeds(seed, B, mu.device)
    out = torch.empty(B, d, device=mu.device, dtype=dt)
    comp = torch.empty(B, device=mu.device, dtype=torch.int32) if return_component else None
    a = L.MixtureSampleArgs()
    a.rows, a.K, a.d, a.mode, a.dtype = B, K, d, mode, L.dtype_code(mc)
    a.pi, a.pi_rs, a.mu, a.mu_rs, a.out, a.out_rs = pc.data_ptr(), K, mc.data_ptr(), K * d, out.data_ptr(), d
    if sc is not None:
        a.sigma, a.sigma_rs = sc.data_ptr(), sigma_len(mode, K, d)
    a.seed = seeds.data_ptr()
    if draw is not None:
        if draw.shape != (B,) or draw.dtype != torch.int64:
            raise ValueError(f"draw must be ({B},) int64")
        _need_cuda(draw)
        draw = draw.contiguous()
        a.draw = draw.data_ptr()
    if use_base:
        a.seed_in = D.device_base(mu.device).data_ptr()
    a.component = L.ptr(comp)
    L.call("mtts_mixture_sample", a)
    return (out, comp) if return_component else out
