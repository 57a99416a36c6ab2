"""The selective-scan backward (scan_bwd_carry_kernel, scan_bwd_kernel,
scan_bwd_reduce) against the float64 oracle at its edge shapes: channel counts
off the 64-channel block, the narrow kernels picked by the shape, ragged L over
several segments, all four (I/O, B/C) dtype pairs, h0 / dh0 across segments,
strided views with poisoned surroundings, a poisoned workspace, and the
numerical edges of softplus, exp2 underflow and slow decay.

The reference always sees the kernel's own (already rounded) inputs:
selective_scan_ref in float64 on the CPU with torch.autograd for the gradients.
Bounds (test_gpu_ops / test_scan_fwd_bwd_c2_shape_vs_oracle): max|err| <=
1e-3 * max|ref| for every fp32 tensor, 1e-2 for the tensors stored as bf16.
The measured errors of every case family are kept in
profiles/scan_bwd_parity.txt (rewritten when MTTS_SCAN_BWD_PARITY names a
file to write)."""

import math
import os

import pytest
import torch

from oracle import mamba_ref as R
from test_gpu_ops import DEV, close

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("bf16", "f32")]
GRADS = ("du", "ddelta", "dz", "dB", "dC", "dA", "dD", "ddelta_bias", "dh0")
BF16_TYPED = ("out", "du", "ddelta", "dz")   # stored in the I/O dtype; everything else is fp32

_ERRS = {}     # family -> tensor name -> max over the family's cases of max|err| / max|ref|
_REFS = {}     # the last oracle result, shared by the segmentings of one case


@pytest.fixture(scope="module", autouse=True)
def _parity_report():
    yield
    path = os.environ.get("MTTS_SCAN_BWD_PARITY")
    if not path or not _ERRS:
        return
    names = ("out", "last_state") + GRADS
    with open(path, "w") as fh:
        fh.write("# tests/test_gpu_scan_bwd.py: max over a family's cases of max|err| / max|ref| per tensor,\n"
                 "# kernel vs the float64 oracle on the same rounded inputs (bounds: 1e-3 fp32 tensors, 1e-2 the\n"
                 "# bf16-stored out / du / ddelta / dz under bf16 I/O and selective_scan_fn's bf16 dB / dC);\n"
                 "# 'segs=3 vs segs=1': the two runs against each other (bound 1e-5 fp32 tensors, 1e-2 bf16-stored)\n")
        fh.write(f"{'family':44s} " + " ".join(f"{n:>11s}" for n in names) + "\n")
        for fam in sorted(_ERRS):
            fh.write(f"{fam:44s} " + " ".join(f"{_ERRS[fam].get(n, float('nan')):11.3e}" for n in names) + "\n")


def _tol(name, io):
    return 1e-2 if io == "bf16" and name in BF16_TYPED else 1e-3


def _check(family, name, got, ref, io, rtol=None):
    """Record the measured relative error, then assert the bound.  A reference
    that is (nearly) zero would leave close()'s 1e-6 scale floor as the only
    check, so it is refused."""
    ref = ref.detach().double().cpu()
    scale = ref.abs().max().item()
    assert math.isfinite(scale) and scale > 1e-4, f"{name}: reference scale {scale:.3e} checks nothing"
    err = (got.detach().double().cpu() - ref).abs().max().item()
    fam = _ERRS.setdefault(family, {})
    fam[name] = max(fam.get(name, 0.0), err / scale) if math.isfinite(err) else float("inf")
    close(got, ref, rtol=rtol or _tol(name, io), name=f"{family} {name}")


def _inputs(B, L, D, io, bc, seed, strided_bc=False):
    """fp32 draws cast to the I/O and B/C dtypes (the oracle gets these rounded
    values).  strided_bc: B / C as column slices of an x_proj-style
    (B, L, 64 + 32) row, as test_gpu_ops._scan_inputs(strided_bc=True)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"u": rn(B, L, D).to(DT[io]), "z": rn(B, L, D).to(DT[io]), "delta": (rn(B, L, D) * 0.5).to(DT[io]),
         "dout": rn(B, L, D).to(DT[io])}
    xd = rn(B, L, 64 + 32).to(DT[bc])
    t["A"] = -torch.exp(rn(D, 16) * 0.5)
    t["D"], t["bias"], t["h0"] = rn(D), rn(D) * 0.1, rn(B, D, 16) * 0.5
    t = {k: v.to(DEV) for k, v in t.items()}
    xd = xd.to(DEV)
    if strided_bc:
        t["B"], t["C"] = xd[..., 64:80], xd[..., 80:96]
    else:
        t["B"], t["C"] = xd[..., 64:80].contiguous(), xd[..., 80:96].contiguous()
    return t


def _oracle(t, softplus=True, a_is_log=False):
    """out, last_state and the nine gradients of sum(out * dout), float64 on the
    CPU, in the kernels' channel-last layout.  a_is_log: t['A'] holds A_log and
    'dA' is the gradient with respect to it."""
    leaf = lambda v: None if v is None else v.detach().double().cpu().requires_grad_()  # noqa: E731
    tr = lambda v: None if v is None else v.transpose(1, 2)  # noqa: E731
    lv = {k: leaf(t.get(k)) for k in ("u", "delta", "z", "B", "C", "A", "D", "bias", "h0")}
    A = -torch.exp(lv["A"]) if a_is_log else lv["A"]
    out, last = R.selective_scan_ref(tr(lv["u"]), tr(lv["delta"]), A, tr(lv["B"]), tr(lv["C"]), lv["D"], tr(lv["z"]),
                                     lv["bias"], delta_softplus=softplus, h0=lv["h0"], return_last_state=True)
    of = dict(zip(GRADS, ("u", "delta", "z", "B", "C", "A", "D", "bias", "h0")))
    names = [n for n in GRADS if lv[of[n]] is not None]
    grads = torch.autograd.grad(out, [lv[of[n]] for n in names], grad_outputs=tr(t["dout"].double().cpu()))
    ref = dict(zip(names, grads))
    ref["out"], ref["last_state"] = out.detach().transpose(1, 2), last.detach()
    assert all(torch.isfinite(v).all() for v in ref.values()), "the oracle itself is not finite on these inputs"
    return ref


def _run(t, softplus=True, a_is_log=False, need_dh0=True, segs=None, path=None, **bwd_kw):
    """scan_fwd (with checkpoints) and scan_bwd under one override: the
    backward's segment count is forced together with the forward's, so the
    checkpoints come from the matching forward."""
    from mtts import _lib, ops
    with _lib.override(scan_path=path, scan_segs=segs, scan_bwd_segs=segs):
        out, last, ckpt = ops.scan_fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t.get("D"), t.get("z"),
                                       t.get("bias"), softplus, h0=t.get("h0"), want_last=True, want_ckpt=True,
                                       a_is_log=a_is_log)
        res = ops.scan_bwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t.get("D"), t.get("z"), t.get("bias"), softplus,
                           t.get("h0"), ckpt, t["dout"], need_dh0=need_dh0, a_is_log=a_is_log, **bwd_kw)
    got = dict(zip(GRADS, res))
    got["out"], got["last_state"] = out, last
    return got


def _compare(family, got, ref, io, t, need_dh0):
    """All of out, last_state and the gradients the case has.  (dD and
    ddelta_bias buffers exist even without D / delta_bias; nothing defines
    them then.)"""
    expect = ["out", "last_state", "du", "ddelta", "dB", "dC", "dA"]
    expect += [n for n, k in (("dz", "z"), ("dD", "D"), ("ddelta_bias", "bias")) if t.get(k) is not None]
    expect += ["dh0"] if need_dh0 else []
    for n in expect:
        assert got[n] is not None, f"{family}: {n} was not returned"
        _check(family, n, got[n], ref[n], io)
    if t.get("z") is None:
        assert got["dz"] is None
    if not need_dh0:
        assert got["dh0"] is None


# ---------------------------------------------------------------------------
# 1. backward vs oracle: shapes x dtype pairs x segmenting x rotated variants
# ---------------------------------------------------------------------------
# Variants toggle one thing of the base case (z, D, delta_bias, softplus, explicit
# A, contiguous B/C, h0 with need_dh0).  Each appears at a narrow shape (D = 3,
# 70; D = 100 under bf16 I/O), at a wide one (D = 192, 136, 200, 64; D = 100
# under fp32 I/O) and with K > 1 segments.  "base" is h0 with need_dh0.
VARIANTS = ("base", "no_z", "no_D", "no_bias", "no_softplus", "a_is_log", "h0_no_dh0", "no_h0", "strided_bc")
SHAPE_VARIANTS = [
    ((1, 1, 1), ("base", "no_softplus")),   # (no h0 at L = 1 would make dA identically zero)
    ((2, 5, 3), ("base", "no_z", "no_D", "no_bias", "a_is_log", "h0_no_dh0", "strided_bc")),
    ((1, 17, 192), ("base", "no_z", "strided_bc")),                   # one step past a chunk
    ((3, 37, 100), ("base", "no_softplus", "a_is_log", "h0_no_dh0")),  # wide for fp32, narrow for bf16
    ((2, 130, 70), VARIANTS),                                         # narrow in both; second block: 6 channels
    ((1, 300, 136), ("base", "no_D", "no_bias", "no_h0")),            # two full blocks + 8 channels; wide
    ((2, 203, 200), ("base", "no_softplus", "h0_no_dh0", "strided_bc")),
    ((2, 1003, 64), ("base", "no_z", "a_is_log")),
]
CASES = [(s, v) for s, vs in SHAPE_VARIANTS for v in vs]
# plan_bwd: seg_len = ceil(ceil(L / K) / 16) * 16, K = ceil(L / seg_len).  (seg_len, K) per forced case:
#   L      segs=2        segs=3                 automatic (K = min(ceil(393216 / (4 B D)), L / 128), at least 1)
#   1      (16, 1)       (16, 1)                (16, 1)
#   5      (16, 1)       (16, 1)                (16, 1)
#   17     (16, 2) 16+1  (16, 2) 16+1           (32, 1)
#   37     (32, 2) 32+5  (16, 3) 16+16+5        (48, 1)
#   130    (80, 2) 80+50 (48, 3) 48+48+34       (144, 1)
#   203    (112, 2) +91  (80, 3) 80+80+43       (208, 1)
#   300    (160, 2) +140 (112, 3) 112+112+76    (160, 2) 160+140
#   1003   (512, 2) +491 (336, 3) 336+336+331   (144, 7) 6*144+139
# Last chunks (steps of the final 16-step chunk): 1 (L = 17), 5 (37), 2 (130), 11 (203, 1003), 12 (300).
SEGS = [None, 2, 3]


def _variant_inputs(shape, variant, io, bc):
    B, L, D = shape
    t = _inputs(B, L, D, io, bc, seed=1000 * VARIANTS.index(variant) + B * L + D,
                strided_bc=variant == "strided_bc")
    softplus, a_is_log, need_dh0 = variant != "no_softplus", variant == "a_is_log", True
    if variant == "no_z":
        del t["z"]
    elif variant == "no_D":
        del t["D"]
    elif variant == "no_bias":
        del t["bias"]
    elif variant == "no_softplus":   # dt is delta + bias itself: keep it positive, as a step size is
        t["delta"] = (t["delta"].float().abs() + 0.4).to(DT[io])
    elif variant == "a_is_log":      # A_log = log(-A)
        t["A"] = torch.log(-t["A"])
    elif variant == "h0_no_dh0":
        need_dh0 = False
    elif variant == "no_h0":
        del t["h0"]
        need_dh0 = False
    return t, softplus, a_is_log, need_dh0


@pytest.mark.parametrize("segs", SEGS, ids=lambda s: f"segs{s or 'auto'}")
@pytest.mark.parametrize("io,bc", PAIRS)
@pytest.mark.parametrize("shape,variant", CASES, ids=[f"{'x'.join(map(str, s))}-{v}" for s, v in CASES])
def test_scan_bwd_vs_oracle(shape, variant, io, bc, segs):
    """All nine results of ops.scan_bwd, plus out and last_state of the forward
    that made its checkpoints, against the float64 oracle.  Nothing forces the
    wide / narrow choice: D % 4 (fp32) or D % 8 (bf16) decides, so both kernels
    run; every launch_bwd<Tio, Tbc> runs at every shape; K is 1, 2, 3 (and 7)
    with ragged last segments and chunks (table above); dh0 ends the
    cross-segment carry chain wherever K > 1."""
    t, softplus, a_is_log, need_dh0 = _variant_inputs(shape, variant, io, bc)
    key = (shape, variant, io, bc)
    if key not in _REFS:
        _REFS.clear()
        _REFS[key] = _oracle(t, softplus, a_is_log)
    got = _run(t, softplus, a_is_log, need_dh0, segs)
    _compare(f"{io}/{bc} segs={segs or 'auto'}", got, _REFS[key], io, t, need_dh0)


# ---------------------------------------------------------------------------
# 2. rows past L and columns outside the views: neither read nor written
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path,segs", [(None, None), (None, 3), (3, None), (3, 3)])
@pytest.mark.parametrize("D", [64, 200])
@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("L", [37, 1003])
def test_scan_bwd_rows_past_L_and_columns_outside_views(L, io, D, path, segs):
    """The layout MambaInnerFn.backward uses: u / delta / dout are [:, :L] row
    views, z is the upper half of an xz row, B / C are columns [64:80] / [80:96]
    of an x_dbl row; everything around the views is NaN.  du / ddelta are row
    views, dz the upper half of dxz, dB / dC columns of an fp32 dx_dbl, all
    inside tensors filled with a sentinel.  Every result must be finite and
    equal, bit for bit, the run on contiguous copies under the same forced path
    (path 3: the narrow kernels), and no sentinel outside the views may change.
    D is a multiple of 8, so every view (row stride D or 2 D, z / dz offset D)
    is 16-byte addressable in both dtypes and wide_bwd_ok answers the same for
    the views as for the contiguous copies."""
    from mtts import _lib, ops
    B, pad, nan = 2, 40, float("nan")
    dt = DT[io]
    t = _inputs(B, L, D, io, io, seed=L + D + (path or 0))

    def big(v, cols=None, at=0, fill=nan):
        bt = torch.full((B, L + pad, cols or v.shape[2]), fill, device=DEV, dtype=v.dtype)
        bt[:, :L, at:at + v.shape[2]] = v
        return bt[:, :L, at:at + v.shape[2]]

    u, dl, dout = big(t["u"]), big(t["delta"]), big(t["dout"])
    z = big(t["z"], 2 * D, D)
    xdbl = torch.full((B, L + pad, 96), nan, device=DEV, dtype=dt)
    xdbl[:, :L, 64:80], xdbl[:, :L, 80:96] = t["B"], t["C"]
    Bm, Cm = xdbl[:, :L, 64:80], xdbl[:, :L, 80:96]
    assert ops._bc_ok(Bm) and ops._bc_ok(Cm)   # passed as they are, not as contiguous copies
    S = 7.0
    du_b = torch.full((B, L + pad, D), S, device=DEV, dtype=dt)
    dd_b = torch.full((B, L + pad, D), S, device=DEV, dtype=dt)
    dxz = torch.full((B, L + pad, 2 * D), S, device=DEV, dtype=dt)
    dx_dbl = torch.full((B, L + pad, 96), S, device=DEV, dtype=torch.float32)
    with _lib.override(scan_path=path, scan_bwd_segs=segs):
        _, _, ckpt = ops.scan_fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["bias"], True,
                                  h0=t["h0"], want_ckpt=True)
        ref = ops.scan_bwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["bias"], True, t["h0"], ckpt,
                           t["dout"], need_dh0=True)
        got = ops.scan_bwd(u, dl, t["A"], Bm, Cm, t["D"], z, t["bias"], True, t["h0"], ckpt, dout,
                           du=du_b[:, :L], ddelta=dd_b[:, :L], dz=dxz[:, :L, D:], dB=dx_dbl[:, :L, 64:80],
                           dC=dx_dbl[:, :L, 80:96], need_dh0=True)
    for n, g, r in zip(GRADS, got, ref):
        assert torch.isfinite(g).all(), f"{n}: a value outside the views was read"
        assert torch.equal(g, r), f"{n}: differs from the run on contiguous copies"
    assert got[0].data_ptr() == du_b.data_ptr() and got[2].data_ptr() == dxz[:, :L, D:].data_ptr()
    for n, bt in (("du", du_b), ("ddelta", dd_b), ("dz", dxz), ("dB/dC", dx_dbl)):
        assert (bt[:, L:] == S).all(), f"{n}: a store landed past row L"
    assert (dxz[:, :, :D] == S).all(), "dz: a store landed in the lower half of dxz"
    assert (dx_dbl[:, :, :64] == S).all(), "dB/dC: a store landed left of the column slices"


# ---------------------------------------------------------------------------
# 3. the workspace is written before it is read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("segs", [None, 3], ids=["segsauto", "segs3"])
@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 37, 70), (1, 300, 136), (2, 1003, 64)])
def test_scan_bwd_workspace_is_write_before_read(shape, io, segs):
    """slab | par | segw arrive uninitialised: with every workspace byte 0xFF
    (each float a NaN) the nine results must stay finite and equal, bit for
    bit, the run on a zeroed workspace -- partial channel blocks, a ragged last
    chunk and the unused segment-0 carry slot included."""
    from mtts import _lib, ops
    B, L, D = shape
    t = _inputs(B, L, D, io, io, seed=B + L + D)
    with _lib.override(scan_segs=segs, scan_bwd_segs=segs):
        n = _lib.lib().mtts_selective_scan_bwd_workspace(B, D, L, 16)
        _, _, ckpt = ops.scan_fwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["bias"], True,
                                  h0=t["h0"], want_ckpt=True)
        res = []
        for fill in (0xFF, 0):
            ws = torch.full((n,), fill, device=DEV, dtype=torch.uint8)
            res.append(ops.scan_bwd(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["bias"], True,
                                    t["h0"], ckpt, t["dout"], need_dh0=True, workspace=ws))
    for name, poisoned, zeroed in zip(GRADS, *res):
        assert torch.isfinite(poisoned).all(), f"{name}: read workspace it had not written"
        assert torch.equal(poisoned, zeroed), f"{name}: depends on the workspace's previous contents"


# ---------------------------------------------------------------------------
# 4. numerical edges
# ---------------------------------------------------------------------------
SOFTPLUS_X = (-30.0, -5.0, 0.0, 19.5, 20.5, 40.0)


@pytest.mark.parametrize("segs", [None, 2], ids=["segsauto", "segs2"])
@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_scan_bwd_softplus_across_threshold(io, segs):
    """delta + delta_bias takes each of -30, -5, 0, 19.5, 20.5, 40 in every
    channel (value (t + c) % 6 at step t of channel c; |bias| <= 0.2 and bf16
    rounding of delta keep 19.5 and 20.5 on their sides of the threshold 20).
    A in [-1, -0.05].  D = 100: wide for fp32, narrow for bf16."""
    B, L, D = 2, 66, 100
    t = _inputs(B, L, D, io, io, seed=66)
    g = torch.Generator().manual_seed(5)
    t["bias"] = ((torch.rand(D, generator=g) * 0.4 - 0.2)).to(DEV)
    t["A"] = -(0.05 + 0.95 * torch.rand(D, 16, generator=g)).to(DEV)
    idx = (torch.arange(L)[:, None] + torch.arange(D)[None]) % len(SOFTPLUS_X)
    x = torch.tensor(SOFTPLUS_X)[idx].to(DEV)
    t["delta"] = (x[None] - t["bias"]).expand(B, L, D).contiguous().to(DT[io])
    seen = (t["delta"].float() + t["bias"])[0]
    for i, v in enumerate(SOFTPLUS_X):
        assert ((seen[idx.to(DEV) == i] - v).abs() < 0.45).all()
    assert (((seen > 20) == (x > 20))).all()
    ref = _oracle(t)
    got = _run(t, segs=segs)
    _compare(f"softplus-threshold {io} segs={segs or 'auto'}", got, ref, io, t, True)


@pytest.mark.parametrize("segs", [None, 3], ids=["segsauto", "segs3"])
@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_scan_bwd_exp_underflow(io, segs):
    """softplus(delta + bias) ~ 8 and A = -16 * 2^U(-4, 1), i.e. A in
    [-32, -1]: exp(dt A) runs from 3e-4 down to exp(-256), which is 0 in fp32
    (v_exp_f32 flushes below 2^-126), so most state pairs forget everything at
    every step while the slowest still carry dA and dh0.  Every gradient must be
    finite (no 0 * inf) and match."""
    B, L, D = 2, 130, 70
    t = _inputs(B, L, D, io, io, seed=130)
    g = torch.Generator().manual_seed(6)
    t["A"] = (-16.0 * torch.exp2(torch.rand(D, 16, generator=g) * 5 - 4)).to(DEV)
    t["delta"] = (8.0 + 0.1 * torch.randn(B, L, D, generator=g)).to(DT[io]).to(DEV)
    ref = _oracle(t)
    got = _run(t, segs=segs)
    _compare(f"exp-underflow {io} segs={segs or 'auto'}", got, ref, io, t, True)


@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_scan_bwd_long_memory_one_vs_three_segments(io):
    """A in [-1e-2, -1e-3] and dt ~ 1e-2 (delta_bias = softplus^-1(1e-2)) at
    L = 1003: a state decays by less than 10 % over the whole sequence, so h0
    (|h0| ~ 1) and, with three segments, the forward carry H_k = exp(A S_{k-1})
    H_{k-1} + h_{k-1} and the backward's reverse carry hold most of every
    result.  One and three segments each match the oracle, and agree with each
    other to 1e-5 of the tensor's range (the forward's split bound) in every
    fp32 tensor.  A tensor stored as bf16 cannot: a 1e-5 difference before
    rounding moves some element by a whole bf16 step (2^-8 of its value), so
    those four keep the bf16 bound 1e-2 between the two runs as well."""
    B, L, D = 2, 1003, 64
    t = _inputs(B, L, D, io, io, seed=1003)
    g = torch.Generator().manual_seed(7)
    t["A"] = -(1e-3 + 9e-3 * torch.rand(D, 16, generator=g)).to(DEV)
    t["bias"] = torch.full((D,), math.log(math.expm1(1e-2)), device=DEV)
    t["delta"] = (0.1 * torch.randn(B, L, D, generator=g)).to(DT[io]).to(DEV)
    t["h0"] = torch.randn(B, D, 16, generator=g).to(DEV)
    ref = _oracle(t)
    one, three = _run(t, segs=1), _run(t, segs=3)
    _compare(f"long-memory {io} segs=1", one, ref, io, t, True)
    _compare(f"long-memory {io} segs=3", three, ref, io, t, True)
    for n in ("out", "last_state") + GRADS:
        _check(f"long-memory {io} segs=3 vs segs=1", n, three[n], one[n], io, rtol=1e-2 if _tol(n, io) > 1e-3 else 1e-5)


# ---------------------------------------------------------------------------
# 5. selective_scan_fn: the upstream signature under autograd
# ---------------------------------------------------------------------------
def test_selective_scan_fn_grads_dtypes_shapes_and_values():
    """(B, D, L) = (2, 70, 37) layout, fp32 u / delta / z with bf16 B / C: each
    gradient has its input's dtype and shape and matches the oracle -- fp32
    tensors at 1e-3; dB / dC come back in bf16 here, whose rounding alone is
    2^-9 of a value, so they take the bf16-stored bound 1e-2."""
    from mtts import ops
    B, D, L = 2, 70, 37
    t = _inputs(B, L, D, "f32", "bf16", seed=70)
    del t["h0"]   # the upstream signature has no initial state
    ref = _oracle(t)
    bdl = lambda v: v.transpose(1, 2).contiguous().requires_grad_()  # noqa: E731
    u, dl, z, Bm, Cm = (bdl(t[k]) for k in ("u", "delta", "z", "B", "C"))
    A, Dp, bias = (t[k].clone().requires_grad_() for k in ("A", "D", "bias"))
    out, last = ops.selective_scan_fn(u, dl, A, Bm, Cm, Dp, z, bias, delta_softplus=True, return_last_state=True)
    assert out.shape == (B, D, L) and out.dtype == torch.float32 and last.shape == (B, D, 16)
    out.backward(t["dout"].transpose(1, 2))
    fam = "selective_scan_fn f32/bf16"
    _check(fam, "out", out.transpose(1, 2), ref["out"], "f32")
    _check(fam, "last_state", last, ref["last_state"], "f32")
    for n, leaf, cl in (("du", u, True), ("ddelta", dl, True), ("dz", z, True), ("dB", Bm, True), ("dC", Cm, True),
                        ("dA", A, False), ("dD", Dp, False), ("ddelta_bias", bias, False)):
        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape, n
        g = leaf.grad.transpose(1, 2) if cl else leaf.grad
        _check(fam, n, g, ref[n], "f32", rtol=1e-2 if leaf.dtype == torch.bfloat16 else 1e-3)
