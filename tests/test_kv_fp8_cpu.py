"""CPU-side checks of the FP8 K/V boundary (mtts_kv_quantize_fp8,
mtts_attention_decode_split_fp8; include/mtts.h): the exported symbols and the
unchanged ABI version, both new structs as the C compiler lays them out
against the ctypes mirrors, the C-side refusals (every check runs before the
first HIP call, so a refused struct touches no device) and the invariants of
the quantiser's reference definition (tests/kv_fp8_ref.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT
from kv_fp8_ref import dequantize_ref, quantize_ref, to_channel_last, to_head_major

HEADER = os.path.join(ROOT, "include", "mtts.h")
EINVAL = -22
_BUF = (C.c_int64 * 64)()            # a host buffer whose address stands for every pointer; never dereferenced
PTR16 = (C.addressof(_BUF) + 15) // 16 * 16   # 16-byte aligned, so that only the fault a row plants is found


def test_symbols_exported_and_abi_unchanged():
    from mtts import _lib
    lib = _lib.lib()
    for name in ("mtts_kv_quantize_fp8", "mtts_kv_quantize_fp8_workspace", "mtts_attention_decode_split_fp8"):
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


@pytest.mark.parametrize("cname,pyname", [("MttsKvQuantizeFp8Args", "KvQuantizeFp8Args"),
                                          ("MttsAttnDecodeSplitFp8Args", "AttnDecodeSplitFp8Args")])
def test_struct_layout_matches_c_header(cname, pyname):
    from mtts import _lib
    cls = getattr(_lib, pyname)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        exe = os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        field, val = line.split()
        got = C.sizeof(cls) if field == "size" else getattr(cls, field).offset
        assert got == int(val), f"{pyname}.{field}: ctypes {got} != C {val}"
        seen += 1
    assert seen == len(cls._fields_) + 1


def test_fp8_attention_args_extend_the_split_args():
    from mtts import _lib
    cls = _lib.AttnDecodeSplitFp8Args
    assert [f for f, _ in cls._fields_] == ["s", "k_scale", "v_scale", "scale_bs"]
    assert cls.s.offset == 0 and cls.s.size == C.sizeof(_lib.AttnDecodeSplitArgs)


def test_quantiser_workspace_is_one_word_per_chunk_of_256_keys():
    from mtts import _lib
    ws = _lib.lib().mtts_kv_quantize_fp8_workspace
    assert ws(3, 2, 64, 1) == ws(3, 2, 64, 256) == 3 * 2 * 4
    assert ws(3, 2, 64, 257) == 3 * 2 * 2 * 4
    assert ws(1, 8, 64, 5248) == 8 * 21 * 4                 # one admitted request: 168 workgroups, not 8
    assert ws(1, 8, 48, 5248) == 0


# -- refusals -----------------------------------------------------------------
def _quant_base():
    from mtts import _lib
    H, hd, S = 2, 64, 5
    return _lib.KvQuantizeFp8Args(rows=1, heads=H, head_dim=hd, kv_len=S, dtype=_lib.BF16, x_bs=S * H * hd,
                                  x_ls=H * hd, out_bs=H * S * hd, scale_bs=H, x=PTR16, kv_lens=None, out=PTR16,
                                  scale=PTR16, workspace=PTR16, workspace_bytes=8)


def _attn_base():
    from mtts import _lib
    H, hd, S = 2, 64, 300
    f = _lib.AttnFwdArgs(batch=1, heads=H, head_dim=hd, q_len=1, kv_len=S, dtype=_lib.BF16, scale=0.125,
                         q_bs=H * hd, q_ls=H * hd, k_bs=H * S * hd, k_ls=hd, v_bs=H * S * hd, v_ls=hd, o_bs=H * hd,
                         o_ls=H * hd, mask_bs=0, q=PTR16, k=PTR16, v=PTR16, key_padding_mask=None, out=PTR16,
                         lse=None, out_packed=None, kv_hs=S * hd)
    s = _lib.AttnDecodeSplitArgs(f=f, kv_lens=None, workspace=PTR16, workspace_bytes=1 * H * 2 * (hd + 2) * 4)
    return _lib.AttnDecodeSplitFp8Args(s=s, k_scale=PTR16, v_scale=PTR16, scale_bs=H)


def _set(a, path, v):
    *head, leaf = path.split(".")
    for h in head:
        a = getattr(a, h)
    setattr(a, leaf, v)


QUANT = "kv_quantize_fp8"
ATTN = "attention_decode_split_fp8"
REFUSALS = [
    (QUANT, None, f"{QUANT}: null args"),
    (QUANT, {"dtype": 2}, f"{QUANT}: dtype must be F32 or BF16"),
    (QUANT, {"head_dim": 48}, f"{QUANT}: head_dim 48 not in {{16,32,64,128}}"),
    (QUANT, {"heads": 0}, f"{QUANT}: bad sizes (rows 1, heads 0, kv_len 5)"),
    (QUANT, {"x": None}, f"{QUANT}: null x / out / scale"),
    (QUANT, {"out": None}, f"{QUANT}: null x / out / scale"),
    (QUANT, {"scale": None}, f"{QUANT}: null x / out / scale"),
    (QUANT, {"x": PTR16 + 8}, f"{QUANT}: x and its strides x_bs / x_ls must be 16-byte aligned"),
    (QUANT, {"x_ls": 132}, f"{QUANT}: x and its strides x_bs / x_ls must be 16-byte aligned"),
    (QUANT, {"out": PTR16 + 4}, f"{QUANT}: out and out_bs must be 8-byte aligned, out_bs >= 640 bytes"),
    (QUANT, {"out_bs": 632}, f"{QUANT}: out and out_bs must be 8-byte aligned, out_bs >= 640 bytes"),
    (QUANT, {"scale_bs": 1}, f"{QUANT}: scale must be 4-byte aligned, scale_bs >= heads = 2"),
    (QUANT, {"kv_lens": PTR16 + 2}, f"{QUANT}: kv_lens must be 4-byte aligned"),
    (QUANT, {"workspace": None}, f"{QUANT}: workspace of 0 bytes, need 8 (4-byte aligned, "
                                 "mtts_kv_quantize_fp8_workspace)"),
    (QUANT, {"workspace_bytes": 4}, f"{QUANT}: workspace of 4 bytes, need 8 (4-byte aligned, "
                                    "mtts_kv_quantize_fp8_workspace)"),
    (ATTN, None, f"{ATTN}: null args"),
    (ATTN, {"s.f.k": None}, f"{ATTN}: null k / v"),
    (ATTN, {"s.f.dtype": 2}, f"{ATTN}: dtype must be F32 or BF16"),
    (ATTN, {"s.f.head_dim": 48}, f"{ATTN}: head_dim 48 not in {{16,32,64,128}}"),
    (ATTN, {"s.f.q_len": 2}, f"{ATTN}: q_len 2 (the single-query kernels take q_len 1)"),
    (ATTN, {"s.workspace_bytes": 1055}, f"{ATTN}: workspace of 1055 bytes, need 1056 (4-byte aligned, "
                                        "mtts_attention_decode_split_workspace)"),
    (ATTN, {"s.workspace": None}, f"{ATTN}: workspace of 0 bytes, need 1056 (4-byte aligned, "
                                  "mtts_attention_decode_split_workspace)"),
    (ATTN, {"s.f.v": PTR16 + 8}, f"{ATTN}: k / v and their strides k_bs / k_ls / v_bs / v_ls / kv_hs must be "
                                 "16-byte aligned"),
    (ATTN, {"s.f.k": PTR16 + 4}, f"{ATTN}: k / v and their strides k_bs / k_ls / v_bs / v_ls / kv_hs must be "
                                 "16-byte aligned"),
    (ATTN, {"s.f.v_ls": 72}, f"{ATTN}: k / v and their strides k_bs / k_ls / v_bs / v_ls / kv_hs must be "
                             "16-byte aligned"),
    (ATTN, {"s.f.kv_hs": 300 * 64 + 8}, f"{ATTN}: k / v and their strides k_bs / k_ls / v_bs / v_ls / kv_hs must be "
                                        "16-byte aligned"),
    (ATTN, {"k_scale": None}, f"{ATTN}: null k_scale / v_scale"),
    (ATTN, {"v_scale": None}, f"{ATTN}: null k_scale / v_scale"),
    (ATTN, {"k_scale": PTR16 + 2}, f"{ATTN}: k_scale / v_scale must be 4-byte aligned, scale_bs >= 0"),
]


@pytest.mark.parametrize("entry,change,message", REFUSALS, ids=[f"{e}-{i}" for i, (e, _, _) in enumerate(REFUSALS)])
def test_refusals_name_the_argument(entry, change, message):
    """Every row MUST fail a check: a struct that passed them all would
    launch a kernel on the host addresses above, so the base structs are
    never called as they are."""
    from mtts import _lib
    lib = _lib.lib()
    fn = getattr(lib, "mtts_" + entry)
    if change is None:
        rc = fn(None, None)
    else:
        a = _quant_base() if entry == QUANT else _attn_base()
        assert change, "a row that changes nothing would launch"
        for path, v in change.items():
            _set(a, path, v)
        rc = fn(C.byref(a), None)
    assert rc == EINVAL
    assert lib.mtts_last_error().decode() == message


# -- the reference's own invariants -------------------------------------------
def _heads(dtype, seed, n=600, S=24, hd=16):
    """n heads as one (n, S, hd) tensor: magnitudes 1e-6 .. 1e6 between heads and a spread inside each."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, 1, 1, generator=g) * 12 - 6)
    spread = 2.0 ** (torch.rand(n, S, hd, generator=g) * -16)
    return (torch.randn(n, S, hd, generator=g) * spread * mag).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_error_bound_and_no_nan(dtype):
    """|deq * scale - x| <= 2^-4 |x| + scale * 2^-10: half an ulp of three
    mantissa bits, and half the subnormal spacing (2^-9 in units of the scale)."""
    x = _heads(dtype, 1)
    q, scale = quantize_ref(x, 1)
    assert torch.isfinite(scale).all() and (scale > 0).all()
    assert ((q & 0x7F) != 0x7F).all(), "a scaled value reached the cast's NaN range"
    xh = to_head_major(x, 1).double()
    err = (dequantize_ref(q, scale) - xh).abs()
    bound = xh.abs() * 2.0 ** -4 + scale.double()[:, :, None, None] * 2.0 ** -10
    ratio = (err / bound).max().item()
    print(f"{dtype}: worst error / bound = {ratio:.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_largest_element_maps_to_the_largest_code(dtype):
    x = _heads(dtype, 2, n=64)
    q, scale = quantize_ref(x, 1)
    xh = to_head_major(x, 1).float()
    flat = xh.abs().flatten(2)
    top = q.flatten(2).gather(2, flat.argmax(2, keepdim=True))
    assert set((top & 0x7F).flatten().tolist()) == {0x7E}   # 448, either sign


def test_reference_zero_head_and_counts():
    H, hd, S = 2, 16, 7
    x = torch.randn(3, S, H * hd)
    x[:, :, :hd] = 0                                        # head 0 of every row is zero
    lens = torch.tensor([0, 3, S + 3], dtype=torch.int32)   # the last one is clamped to S
    q, scale = quantize_ref(x, H, lens)
    assert q.shape == (3, H, S, hd) and q.dtype == torch.uint8 and scale.shape == (3, H)
    assert (scale[:, 0] == 1).all() and (q[:, 0] == 0).all()
    assert scale[0, 1] == 1 and (q[0] == 0).all()           # no counted key at all
    assert (q[1, :, 3:] == 0).all() and (q[1, 1, :3] != 0).any()
    full, fscale = quantize_ref(x[2:], H)
    assert torch.equal(q[2:], full) and torch.equal(scale[2:], fscale)
    # a key past the count does not enter the scale
    y = x.clone()
    y[1, 3:] *= 1000
    q2, s2 = quantize_ref(y, H, lens)
    assert torch.equal(q2[1], q[1]) and torch.equal(s2[1], scale[1])
    assert torch.equal(to_channel_last(to_head_major(x, H)), x)


def test_reference_non_finite_gives_nan_scale():
    x = torch.randn(1, 4, 32)
    x[0, 1, 3] = float("inf")
    x[0, 2, 20] = float("nan")
    _, scale = quantize_ref(x, 2)
    assert torch.isnan(scale).all()
    _, scale = quantize_ref(x, 2, torch.tensor([1], dtype=torch.int32))
    assert torch.isfinite(scale).all()
