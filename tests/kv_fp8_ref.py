"""CPU reference of the FP8 K/V quantiser (mtts_kv_quantize_fp8,
include/mtts.h): the definition with torch's own float8_e4m3fn cast, the
dequantiser and the head-major <-> channel-last reshapes.  Everything here
runs on CPU tensors; the GPU tests move the kernels' results over."""
import torch

FP8_MAX = 448.0                      # the largest finite e4m3fn value
NAN_CODE = 0x7F                      # e4m3fn has no infinity: 0x7F / 0xFF are its NaN


def to_head_major(x, H):
    """(R, S, H * hd) channel-last -> (R, H, S, hd) contiguous."""
    R, S, d = x.shape
    return x.reshape(R, S, H, d // H).permute(0, 2, 1, 3).contiguous()


def to_channel_last(xh):
    """(R, H, S, hd) head-major -> (R, S, H * hd) contiguous."""
    R, H, S, hd = xh.shape
    return xh.permute(0, 2, 1, 3).reshape(R, S, H * hd).contiguous()


def clamp_counts(kv_lens, R, S):
    if kv_lens is None:
        return torch.full((R,), S, dtype=torch.int64)
    return kv_lens.to(torch.int64).clamp(0, S)


def quantize_ref(x, H, kv_lens=None):
    """x (R, S, H * hd) bf16 / fp32 on the CPU -> (bytes (R, H, S, hd) uint8,
    scale (R, H) fp32): scale = max |x| over the head's columns of the row's
    first n_r keys / 448 in fp32 (1 where that max is 0, NaN where it is not
    finite), bytes = (x.float() / scale).to(float8_e4m3fn) for keys below the
    count and 0 from it on."""
    x = x.detach().cpu()
    R, S, _ = x.shape
    xh = to_head_major(x.float(), H)                                    # (R, H, S, hd)
    n = clamp_counts(kv_lens, R, S)
    counted = (torch.arange(S)[None, :] < n[:, None])[:, None, :, None]  # (R, 1, S, 1)
    mag = torch.where(counted, xh.abs(), torch.zeros(()))
    amax = mag.amax(dim=(2, 3)) if S else torch.zeros(R, H)
    amax = torch.where(torch.isnan(mag).any(-1).any(-1), torch.full((), float("nan")), amax)
    scale = torch.where(amax == 0, torch.ones(()), amax / torch.tensor(FP8_MAX, dtype=torch.float32))
    scale = torch.where(torch.isfinite(amax), scale, torch.full((), float("nan")))
    q = (xh / scale[:, :, None, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where(counted, q, torch.zeros((), dtype=torch.uint8))
    return q.contiguous(), scale.contiguous()


def dequantize_ref(q, scale, dtype=torch.float64):
    """bytes (R, H, S, hd) uint8 and scale (R, H) -> deq(bytes) * scale,
    (R, H, S, hd) in `dtype`; every e4m3fn value and an fp32 scale are exact
    in float64, and so is their product."""
    return q.detach().cpu().view(torch.float8_e4m3fn).to(dtype) * scale.detach().cpu().to(dtype)[:, :, None, None]
