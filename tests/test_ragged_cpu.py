"""Boundary of the ragged-prompt feature, checked without a GPU: the new
entry point is exported and bound, the public signatures carry the new
keywords, the appended struct fields sit where the C compiler puts them, and
the ABI number did not move (the change is additive)."""
import ctypes
import inspect
import os
import subprocess
import tempfile

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mtts.h")


def test_library_exports_embed_sum_at_and_abi_is_still_15():
    from mtts import _lib
    lib = _lib.lib()
    assert hasattr(lib, "mtts_embed_sum_at") and "mtts_embed_sum_at" in _lib.exported_symbols()
    assert hasattr(lib, "mtts_embed_sum")                      # the old entry point stays
    assert len(lib.mtts_embed_sum_at.argtypes) == len(lib.mtts_embed_sum.argtypes) + 2
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


def test_signatures_carry_the_new_keywords():
    import mamba_decoder
    from mtts import ops
    from mtts.decode import DecodeEngine
    from mtts.mamba import Mamba

    def has(fn, name):
        p = inspect.signature(fn).parameters
        return name in p and p[name].default is None

    assert has(mamba_decoder.MambaTTSDecoder.generate, "prompt_lengths")
    assert has(DecodeEngine.generate, "prompt_lengths")
    assert has(Mamba.forward, "seq_lens")
    assert has(ops.scan_fwd, "seq_lens")
    assert has(ops.conv_fwd, "seq_lens")
    assert has(mamba_decoder.MambaTTSDecoderLayer.forward_fused, "seq_lens")
    assert has(mamba_decoder.MambaTTSDecoder._run_layers, "seq_lens")
    # the reference signatures only gained trailing optional arguments
    assert list(inspect.signature(Mamba.forward).parameters)[:3] == ["self", "x", "state"]
    gen = list(inspect.signature(mamba_decoder.MambaTTSDecoder.generate).parameters)
    assert gen[:4] == ["self", "text_hidden", "z_style", "max_new_tokens"]


def test_appended_fields_are_last_and_match_the_header():
    """seqlens is the LAST field of both forward structs (a caller that zero-
    fills the struct keeps the old behaviour) and pos_rows took the slot of the
    sampler's reserved int: offsets and sizes against the C compiler."""
    from mtts import _lib
    assert _lib.ScanFwdArgs._fields_[-1][0] == "seqlens"
    assert _lib.ConvFwdArgs._fields_[-1][0] == "seqlens"
    names = [f for f, _ in _lib.SampleArgs._fields_]
    assert "pos_rows" in names and "reserved_" not in names
    assert names[names.index("pos_rows") - 1] == "pad_id" and names[names.index("pos_rows") + 1] == "finished"
    probes = [("MttsScanFwdArgs", _lib.ScanFwdArgs, "seqlens"), ("MttsConvFwdArgs", _lib.ConvFwdArgs, "seqlens"),
              ("MttsSampleArgs", _lib.SampleArgs, "pos_rows")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, _, field in probes:
        lines.append(f'printf("%zu %zu\\n", sizeof({cname}), offsetof({cname}, {field}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    for i, (cname, py, field) in enumerate(probes):
        assert ctypes.sizeof(py) == int(out[2 * i]), cname
        assert getattr(py, field).offset == int(out[2 * i + 1]), (cname, field)
    # the sampler struct kept its size and the offset of everything behind the renamed field (ABI 15 as released)
    assert ctypes.sizeof(_lib.SampleArgs) == 160 and _lib.SampleArgs.pos_rows.offset == 132


def test_a_library_from_before_the_additions_is_refused_by_name(monkeypatch):
    """ABI 15 grew by additions only, so a stale build also reports 15: the
    loader must say so itself instead of failing later inside ctypes."""
    import pytest
    from mtts import _lib
    with tempfile.TemporaryDirectory() as d:
        c, so = os.path.join(d, "stale.c"), os.path.join(d, "libstale.so")
        open(c, "w").write("int mtts_abi_version(void) { return 15; }\n")
        subprocess.run(["gcc", "-shared", "-fPIC", c, "-o", so], check=True)
        monkeypatch.setattr(_lib, "LIB_PATH", so)
        monkeypatch.setattr(_lib, "_lib", None)
        with pytest.raises(RuntimeError, match="mtts_embed_sum_at"):
            _lib.lib()
