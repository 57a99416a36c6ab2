"""The owner of a decode context's per-request rows (mtts/conditioning.py):
its row operations against its own build-from-batch constructor, bit for bit,
in every format -- fp32 generic (row-major K / V only), bf16 packed (row-major,
head-major and packed FiLM; opened shared, so with kv_rows) and bf16 with FP8
keys -- the purity of the engine's packed-step predicate, and the texts of the
errors the two split-key wrappers raise through their common front end.

The decoder is that of test_gpu_long_keys.py (2 layers, d_model 512, 8 heads:
head dim 64, 256 keys per chunk, KEYS = 520); 4 rows, one request of 300 keys
whose mask has a hole below the count."""
import pytest
import torch

from test_gpu_generate import DEV
from test_gpu_long_keys import DM, DS, HEADS, KEYS, _decoder

pytestmark = pytest.mark.gpu
ROWS, COUNT = 4, 300
FORMATS = {"fp32": (None, None, False), "bf16": (torch.bfloat16, None, True), "fp8": (torch.bfloat16, "fp8", False)}
FILM, PACKED_FILM = {"gamma", "beta"}, {"gamma_p", "beta_p"}
EXISTS = {"fp32": {"k", "v"} | FILM, "bf16": {"k", "v", "khm", "vhm"} | FILM | PACKED_FILM,
          "fp8": {"k8", "v8", "k_scale", "v_scale"} | FILM | PACKED_FILM}
ROW_IMAGES = ("k", "v", "khm", "vhm", "k8", "v8", "k_scale", "v_scale", "gamma", "beta")
_models = {}


def _setup(fmt):
    """The format's model, and `make`: a Conditioning and the context over it, routed unless told otherwise -- the
    idle rows, or built from the conditioning batch given."""
    from mtts.conditioning import Conditioning
    from mtts.context import DecodeContext
    cd, kv_dtype, shared = FORMATS[fmt]
    if cd not in _models:
        _models[cd] = _decoder(cd)
    m = _models[cd]

    def make(batch=None, latch=True):
        with torch.no_grad():
            if batch is None:
                cond = Conditioning.idle(ROWS, KEYS, m._cd(), torch.device(DEV), kv_dtype, True, shared)
            else:
                th, keep, z = batch
                cond = Conditioning.from_batch(m, th, z, keep, None, None, m._cd(), kv_dtype, True)
            ctx = DecodeContext(m, cond)
            if latch:
                ctx.latch(cond.rows)
                assert ctx.xpk == (fmt != "fp32")
        return cond, ctx

    return m, make


def _request(m):
    """The request padded to KEYS keys at batch 1, as an admission pads it: (th, keep, z)."""
    g = torch.Generator().manual_seed(77)
    th = torch.zeros(1, KEYS, DM)
    th[0, :COUNT] = torch.randn(COUNT, DM, generator=g)
    keep = torch.zeros(1, KEYS, dtype=torch.bool)
    keep[0, :COUNT] = True
    keep[0, 100:131] = False
    return th.to(DEV).to(m._cd()), keep.to(DEV), torch.randn(1, DS, generator=g).to(DEV)


def _row(cond, r):
    """Every stored image of row r, by name (None: the image does not exist)."""
    out = {"kpm": cond.kpm[r], "kv_lens": cond.kv_lens[r]}
    for i, c in enumerate(cond.layers):
        for name in ROW_IMAGES:
            t = getattr(c, name)
            out[f"{i}.{name}"] = None if t is None else t[r]
        for name in ("gamma_p", "beta_p"):
            p = getattr(c, name)
            out[f"{i}.{name}"] = None if p is None else p.unpack()[r]
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert (a[name] is None) == (b[name] is None), f"{what}: {name} exists in one only"
        assert a[name] is None or torch.equal(a[name], b[name]), f"{what}: {name} differs"


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_write_equals_build(fmt):
    m, make = _setup(fmt)
    th, keep, z = _request(m)
    cond, _ = make()
    idle = [_row(cond, r) for r in range(ROWS)]
    with torch.no_grad():
        cond.write(2, th, keep, z)
    built, _ = make((th, keep, z))
    got = _row(cond, 2)
    for c in cond.layers:                                   # the comparison below covers every image of the format
        assert {n for n in ROW_IMAGES + ("gamma_p", "beta_p") if getattr(c, n) is not None} == EXISTS[fmt]
    assert int(cond.kv_lens[2]) == COUNT and not bool(cond.kpm[2, 99]) and bool(cond.kpm[2, 100])
    _assert_same(got, _row(built, 0), "row 2 against the row built from the batch")
    for r in (0, 1, 3):
        _assert_same(_row(cond, r), idle[r], f"row {r} is still idle")


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_idle_is_idle(fmt):
    m, make = _setup(fmt)
    cond, _ = make()
    fresh, _ = make()
    with torch.no_grad():
        cond.write(2, *_request(m))
        cond.point(2, 1)
        assert int(cond.kv_lens[2]) == COUNT
        cond.clear(2)
    for r in range(ROWS):
        _assert_same(_row(cond, r), _row(fresh, r), f"row {r} against a fresh idle row")
    assert cond.kv_lens.tolist() == [1] * ROWS and cond.kpm[:, 1:].all() and not cond.kpm[:, 0].any()
    if fmt == "fp8":
        assert all((c.k_scale == 1).all() and (c.v_scale == 1).all() and not c.k8.any() for c in cond.layers)
    if FORMATS[fmt][2]:
        assert cond.kv_rows.tolist() == list(range(ROWS))
    else:
        assert cond.kv_rows is None


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_copy_is_copy(fmt):
    m, make = _setup(fmt)
    cond, _ = make()
    with torch.no_grad():
        cond.write(2, *_request(m))
        cond.copy(2, 0)
    _assert_same(_row(cond, 0), _row(cond, 2), "row 0 against row 2")
    assert int(cond.kv_lens[0]) == COUNT


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_the_routing_predicate_is_pure(fmt):
    m, make = _setup(fmt)
    from mtts.context import fused_ok
    cond, ctx = make(latch=False)
    ctx.fused = fused_ok(m, cond.cd, ROWS, True)
    ctx.pack_weights()
    assert ctx.fused and ctx.xpk_ok() is True and ctx.xpk_ok() is True
    assert all(t is None for c in cond.layers for t in (c.khm, c.vhm, c.gamma_p, c.beta_p))
    assert ctx.fuse_q_ok(ROWS) is False                    # 520 keys: past the single-pass range; it reads no image
    cond.make_packed_images()
    assert all(c.gamma_p is not None and c.beta_p is not None for c in cond.layers)
    assert all((c.khm is not None and c.vhm is not None) == (fmt == "bf16") for c in cond.layers)


B, S, HD = 3, 300, DM // HEADS


def _split_call(fp8, **bad):
    """attention_decode_split (fp8: its fp8 form) on valid operands, `bad` replacing some."""
    from mtts import attn_kernels as A
    q = torch.zeros(B, DM, device=DEV, dtype=torch.bfloat16)
    kw = dict(kpm=None, kv_lens=torch.full((B,), S, dtype=torch.int32, device=DEV), workspace=None)
    if fp8:
        ops = dict(k8=torch.zeros(B, HEADS, S, HD, device=DEV, dtype=torch.uint8),
                   k_scale=torch.ones(B, HEADS, device=DEV))
        ops.update({n: bad.pop(n) for n in list(bad) if n in ops})
        kw.update(bad)
        return A.attention_decode_split_fp8(q, ops["k8"], ops["k8"], ops["k_scale"], ops["k_scale"], HEADS, **kw)
    k = bad.pop("k", torch.zeros(B, S, DM, device=DEV, dtype=torch.bfloat16))
    kw.update(bad)
    return A.attention_decode_split(q, k, k, HEADS, **kw)


def _errors():
    both = {"kv_lens": (lambda fp8: dict(kv_lens=torch.full((B,), S, dtype=torch.int64, device=DEV)),
                        ValueError, f"{{who}}: kv_lens must be \\({B},\\) int32 on the device"),
            "workspace": (lambda fp8: dict(workspace=torch.empty(4, dtype=torch.uint8, device=DEV)),
                          ValueError, "{who}: workspace must be >= [0-9]+ contiguous uint8 bytes on the device"),
            "empty": (lambda fp8: ({"k8": torch.zeros(B, HEADS, 0, HD, device=DEV, dtype=torch.uint8)} if fp8 else
                                   {"k": torch.zeros(B, 0, DM, device=DEV, dtype=torch.bfloat16)}),
                      ValueError, "{who}: the key side is empty")}
    cases = [pytest.param(fp8, *both[n], id=f"{n}-{'fp8' if fp8 else 'split'}") for n in both for fp8 in (False, True)]
    cases += [
        pytest.param(False, lambda fp8: dict(kv_rows=torch.zeros(B, dtype=torch.int64, device=DEV)), ValueError,
                     f"{{who}}: kv_rows must be \\({B},\\) int32 on the device", id="kv_rows-split"),
        pytest.param(True, lambda fp8: dict(k_scale=torch.ones(B, HEADS + 1, device=DEV)), ValueError,
                     f"{{who}}: k_scale must be \\({B}, {HEADS}\\) fp32, contiguous", id="scale-fp8"),
        pytest.param(True, lambda fp8: dict(k8=torch.zeros(B, HEADS, S, HD, device=DEV, dtype=torch.int8)), TypeError,
                     "{who}: k8 / v8 must be \\(B, H, S, hd\\) torch.uint8", id="bytes-fp8")]
    return cases


@pytest.mark.parametrize("fp8, bad, exc, text", _errors())
def test_split_wrapper_errors_keep_their_texts(fp8, bad, exc, text):
    who = "attention_decode_split_fp8" if fp8 else "attention_decode_split"
    with pytest.raises(exc, match="^" + text.format(who=who)):
        _split_call(fp8, **bad(fp8))
