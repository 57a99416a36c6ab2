"""CPU-side checks of the parallel-samples feature: the shared-key attention's
boundary (mtts_attention_decode_split_shared, include/mtts.h: the exported
symbol, the unchanged ABI version, MttsAttnDecodeSplitSharedArgs as the C
compiler lays it out against the ctypes mirror), plan_slots with `samples`,
and the checks of admit_samples that need no device."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mtts.h")


def test_symbol_exported_and_abi_unchanged():
    from mtts import _lib
    lib = _lib.lib()
    name = "mtts_attention_decode_split_shared"
    assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


def test_shared_args_layout_matches_c_header():
    from mtts import _lib
    cls = _lib.AttnDecodeSplitSharedArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(MttsAttnDecodeSplitSharedArgs));',
             'printf("inner %zu\\n", sizeof(MttsAttnDecodeSplitArgs));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(MttsAttnDecodeSplitSharedArgs, {fname}));')
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
        if field == "size":
            got = ctypes.sizeof(cls)
        elif field == "inner":                               # the embedded struct is the existing one, unchanged
            got = ctypes.sizeof(_lib.AttnDecodeSplitArgs)
        else:
            got = getattr(cls, field).offset
        assert got == int(val), f"AttnDecodeSplitSharedArgs.{field}: ctypes {got} != C {val}"
        seen += 1
    assert seen == len(cls._fields_) + 2
    assert [f for f, _ in cls._fields_] == ["s", "kv_rows", "kv_batch"]
    assert cls.s.offset == 0 and cls.s.size == ctypes.sizeof(_lib.AttnDecodeSplitArgs)
    assert [f for f, _ in _lib.AttnDecodeSplitArgs._fields_] == ["f", "kv_lens", "workspace", "workspace_bytes"]


CASES = [([5, 3, 9, 2, 2], 2, 4, None), ([5, 3, 9, 2, 2], 2, 4, [0, 1, 0, 0, 1]), ([1, 1, 1], 1, 16, None),
         ([7, 20, 3, 3, 3, 11], 3, 5, [1, 0, 0, 1, 0, 0]), ([4] * 9, 4, 3, None)]


def _plan_before(caps, slots, check_every, prefilled=None):
    """plan_slots as it was before `samples`: what the answers without it must stay."""
    pre = [False] * len(caps) if prefilled is None else [bool(p) for p in prefilled]
    left = [None] * slots
    where, nxt, replays = [], 0, 0
    while nxt < len(caps) or any(v is not None for v in left):
        for s in range(slots):
            if left[s] is None and nxt < len(caps):
                left[s] = caps[nxt] - (1 if pre[nxt] else 0)
                where.append(s)
                nxt += 1
        n = min(check_every, max(v for v in left if v is not None))
        replays += n
        left = [None if v is None or v - n <= 0 else v - n for v in left]
    return where, replays


@pytest.mark.parametrize("caps,slots,every,pre", CASES)
def test_plan_slots_without_samples_is_unchanged(caps, slots, every, pre):
    from mtts.session import plan_slots
    want = _plan_before(caps, slots, every, pre)
    assert plan_slots(caps, slots, every, pre) == want
    assert plan_slots(caps, slots, every, pre, samples=None) == want
    assert plan_slots(caps, slots, every, pre, samples=[None] * len(caps)) == want


def test_plan_slots_with_samples():
    from mtts.session import plan_slots
    # 4 slots, one check per 4 tokens.  Request 1 (3 samples) finds slots 1-3 idle beside request 0; request 2
    # (2 samples) takes the two lowest of them once they are idle again, request 3 the one that is left.
    where, replays = plan_slots([8, 4, 4, 2], 4, 4, samples=[None, 3, 2, None])
    assert where == [0, [1, 2, 3], [1, 2], 3]
    # round 1: 0 and 1,2,3 live, 4 replays: the group is done, request 0 has 4 left.  round 2: request 2 into 1, 2,
    # request 3 into 3; 4 replays end everything
    assert replays == 8
    # blocking in order: request 1 (4 samples) needs every slot, so request 2 (one slot free all along) waits
    where, replays = plan_slots([6, 2, 2], 4, 2, samples=[None, 4, None])
    assert where == [0, [0, 1, 2, 3], 0] and replays == 6 + 2 + 2
    # samples = 1 answers with a list of one slot, the lowest idle one
    assert plan_slots([3, 3], 2, 8, samples=[1, None])[0] == [[0], 1]
    # prefilled members need one replay less, every one of them
    assert plan_slots([5], 3, 8, [True], samples=[3]) == ([[0, 1, 2]], 4)
    for bad in ([5], [0], [None, -1]):
        with pytest.raises(ValueError, match="samples"):
            plan_slots([3] * len(bad), 4, 4, samples=bad)
    with pytest.raises(ValueError, match="samples"):
        plan_slots([3, 3], 4, 4, samples=[1])


def test_admit_samples_checks_its_slots_first():
    """The slot-list checks run before the session or the device is touched:
    an object with nothing but a slot count gets through them."""
    from mtts.session import DecodeSession
    ses = object.__new__(DecodeSession)
    ses.slots = 4
    for bad in ([], (), "01", None, 3):
        with pytest.raises(ValueError, match="list of one or more distinct slots"):
            ses.admit_samples(bad, None, None, max_new_tokens=1)
    with pytest.raises(ValueError, match="distinct"):
        ses.admit_samples([1, 2, 1], None, None, max_new_tokens=1)
    for bad in ([0, 4], [-1], [True], [1.0]):
        with pytest.raises(ValueError, match="slot must be an integer"):
            ses.admit_samples(bad, None, None, max_new_tokens=1)
    with pytest.raises(AttributeError):                      # past them: the first use of the session's state
        ses.admit_samples([0, 1], None, None, max_new_tokens=1)
