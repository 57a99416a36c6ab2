"""CPU-side checks of the split-key single-query attention's boundary
(mtts_attention_decode_split, include/mtts.h): the exported symbols and the
unchanged ABI version, MttsAttnDecodeSplitArgs as the C compiler lays it out
against the ctypes mirror, the chunk size per head dim and key_counts, the
one definition of a row's key count."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mtts.h")


def test_symbols_exported_and_abi_unchanged():
    from mtts import _lib
    lib = _lib.lib()
    for name in ("mtts_attention_decode_split", "mtts_attention_decode_split_workspace"):
        assert hasattr(lib, name) and name in _lib.exported_symbols(), name
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


def test_split_args_layout_matches_c_header():
    from mtts import _lib
    cls = _lib.AttnDecodeSplitArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(MttsAttnDecodeSplitArgs));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(MttsAttnDecodeSplitArgs, {fname}));')
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
        got = ctypes.sizeof(cls) if field == "size" else getattr(cls, field).offset
        assert got == int(val), f"AttnDecodeSplitArgs.{field}: ctypes {got} != C {val}"
        seen += 1
    assert seen == len(cls._fields_) + 1
    assert [f for f, _ in cls._fields_] == ["f", "kv_lens", "workspace", "workspace_bytes"]
    assert cls.f.offset == 0 and cls.f.size == ctypes.sizeof(_lib.AttnFwdArgs)


def test_workspace_is_one_partial_per_chunk():
    from mtts import _lib
    from mtts.attn_kernels import decode_split_chunk
    ws = _lib.lib().mtts_attention_decode_split_workspace
    for hd in (16, 32, 64, 128):
        ck = decode_split_chunk(hd)
        per = (hd + 2) * 4                                   # chunk max, sum p, hd accumulators, fp32
        assert ws(3, 2, hd, 1) == ws(3, 2, hd, ck) == 3 * 2 * per
        assert ws(3, 2, hd, ck + 1) == ws(3, 2, hd, 2 * ck) == 3 * 2 * 2 * per
    assert ws(1, 8, 64, 5248) == 8 * 21 * 66 * 4


def test_chunk_per_head_dim():
    from mtts.attn_kernels import decode_split_chunk
    assert [decode_split_chunk(hd) for hd in (128, 64, 32, 16)] == [128, 256, 512, 1024]
    with pytest.raises(ValueError, match="head_dim"):
        decode_split_chunk(48)


def test_key_counts_on_the_cpu():
    from mtts.attn_kernels import key_counts
    S = 12
    keep = torch.zeros(5, S, dtype=torch.bool)
    keep[0, :7] = True                                       # no holes
    keep[1, :3] = True                                       # [ref ‖ text]: the reference's padding is a hole
    keep[1, 5:9] = True
    #     row 2 keeps nothing
    keep[3, :] = True                                        # every key
    keep[4, S - 1] = True                                    # the last key alone
    n = key_counts(keep)
    assert n.dtype == torch.int32 and n.shape == (5,)
    assert n.tolist() == [7, 9, 0, S, S]
    assert key_counts(torch.zeros(2, 0, dtype=torch.bool)).tolist() == [0, 0]
    with pytest.raises(TypeError):
        key_counts(keep.to(torch.uint8))
