"""Per-row valid lengths through the kernels (a ragged, right-padded batch):
the selective scan forward stops each row at its own length, the causal conv
leaves the window ending there, mtts_embed_sum_at embeds a per-row position
and the sampler's advance launch moves B position counters.  References: the
float64 oracle run per row on the truncated input (scan), torch gathers (conv,
embedding)."""
import functools

import pytest
import torch

from oracle import mamba_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENS = lambda L: [L, 1, 0, 15, 16, 17]  # noqa: E731  either side of the 8- and 16-step tile edges
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _rel(out, ref):
    ref = ref.double().cpu()
    return (out.double().cpu() - ref).abs().max().item(), max(ref.abs().max().item(), 1e-6)


@functools.lru_cache(maxsize=None)
def _scan_case(B, D, L, io):
    """Inputs (already rounded to the I/O dtype, NaN at t >= len_b) and the
    float64 oracle per row on the truncated row, with and without h0; made
    once per shape and dtype and shared by every kernel configuration."""
    dt = DT[io]
    g = torch.Generator().manual_seed(B * L + D)
    u = torch.randn(B, L, D, generator=g).to(dt)
    z = torch.randn(B, L, D, generator=g).to(dt)
    dl = (torch.randn(B, L, D, generator=g) * 0.5).to(dt)
    Bm = torch.randn(B, L, 16, generator=g).to(dt)
    Cm = torch.randn(B, L, 16, generator=g).to(dt)
    A = -torch.exp(torch.randn(D, 16, generator=g) * 0.5)
    Dp = torch.randn(D, generator=g)
    bias = torch.randn(D, generator=g) * 0.1
    h0 = torch.randn(B, D, 16, generator=g) * 0.5
    lens = LENS(L)
    refs = {}
    for with_h0 in (False, True):
        out = torch.zeros(B, L, D, dtype=torch.float64)
        last = torch.zeros(B, D, 16, dtype=torch.float64)
        for b, n in enumerate(lens):
            hb = h0[b:b + 1].double() if with_h0 else None
            if n == 0:
                last[b] = 0.0 if hb is None else hb[0]
                continue
            cut = lambda t: t[b:b + 1, :n].double().transpose(1, 2)  # noqa: E731
            o, l = R.selective_scan_ref(cut(u), cut(dl), A.double(), cut(Bm), cut(Cm), Dp.double(), cut(z),
                                        bias.double(), delta_softplus=True, h0=hb, return_last_state=True)
            out[b, :n] = o[0].transpose(0, 1)
            last[b] = l[0]
        refs[with_h0] = (out, last)
    valid = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]           # (B, L)
    nan = float("nan")
    for t in (u, dl, z, Bm, Cm):
        t[~valid] = nan
    dev = lambda t: t.to(DEV)  # noqa: E731
    return tuple(map(dev, (u, dl, A, Bm, Cm, Dp, z, bias, h0))), lens, valid, refs


def _run_ragged(inputs, lens, with_h0, **kw):
    from mtts import ops
    u, dl, A, Bm, Cm, Dp, z, bias, h0 = inputs
    out = torch.full_like(u, 7.0)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    out, last, _ = ops.scan_fwd(u, dl, A, Bm, Cm, Dp, z, bias, True, h0=h0 if with_h0 else None, want_last=True,
                                out=out, seq_lens=sl, **kw)
    return out, last


CONFIGS = [dict(scan_p=2), dict(scan_p=4), dict(scan_p=2, scan_segs=3), dict(scan_p=4, scan_segs=3)]
PATHS = [dict(scan_path=1), dict(scan_path=2), dict(scan_path=2, scan_p=2, scan_segs=3)]


def _id(o):
    return "-".join(f"{k[5:]}{v}" for k, v in o.items())


@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero", "h0"])
@pytest.mark.parametrize("shape,ovr", [((6, 64, 37), o) for o in CONFIGS + PATHS] + [((6, 70, 130), o) for o in CONFIGS],
                         ids=lambda v: _id(v) if isinstance(v, dict) else "x".join(map(str, v)))
def test_scan_seq_lens_vs_oracle_per_row(shape, ovr, with_h0, io):
    """out[b, :len_b] and last_state[b] against the oracle on the row cut to
    len_b steps; every input at t >= len_b is NaN (nothing there may reach a
    result) and out[b, len_b:] keeps its sentinel (nothing there is written).
    P = 2 / 4, L forced into 3 segments (identity segments past a row's end),
    and the one-lane / LDS-DMA overrides, which a ragged call must route to
    the generic kernel."""
    from mtts import _lib
    B, D, L = shape
    inputs, lens, valid, refs = _scan_case(B, D, L, io)
    with _lib.override(**ovr):
        out, last = _run_ragged(inputs, lens, with_h0)
    ref_out, ref_last = refs[with_h0]
    v = valid.to(DEV)
    assert torch.isfinite(out[v]).all() and torch.isfinite(last).all()
    assert (out[~v] == 7.0).all(), "a store landed at t >= len_b"
    got = torch.where(v[:, :, None], out.float(), torch.zeros((), device=DEV))
    eo, so = _rel(got, ref_out)
    el, sl_ = _rel(last, ref_last)
    tol = 1e-3 if io == "f32" else 1e-2   # the bounds of tests/test_gpu_ops.py (bf16: output rounding)
    print(f"{shape} {ovr} h0={with_h0} {io}: out {eo:.3e} / {so:.3e}, last {el:.3e} / {sl_:.3e}")
    assert eo <= tol * so, (eo, so)
    assert el <= 1e-3 * sl_, (el, sl_)
    for b, n in enumerate(lens):   # per row too: a short row must not hide behind a long row's scale
        if n:
            e, s = _rel(got[b, :n], ref_out[b, :n])
            assert e <= tol * s, (b, n, e, s)
        e, s = _rel(last[b], ref_last[b])
        assert e <= 1e-3 * max(s, 1e-3), (b, n, e, s)


def test_scan_seq_lens_rejects_checkpoints():
    from mtts import _lib, ops
    inputs, lens, _, _ = _scan_case(6, 64, 37, "f32")
    with pytest.raises(ValueError):
        _run_ragged(inputs, lens, False, want_ckpt=True)
    # and at the C boundary: ckpt together with seqlens is MTTS_EINVAL
    u, dl, A, Bm, Cm, Dp, z, bias, h0 = (t.nan_to_num(0.0) if t.is_floating_point() else t for t in inputs)
    out, ck = torch.empty_like(u), torch.empty(6, 3, 64, 16, device=DEV)
    a = ops._scan_args(u, dl, A, Bm, Cm, Dp, z, bias, True, None, out, None, ck)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    a.seqlens = sl.data_ptr()
    with pytest.raises(RuntimeError, match="seqlens"):
        _lib.call("mtts_selective_scan_fwd", a)


@pytest.mark.parametrize("ovr", [dict(), dict(scan_p=2, scan_segs=3)], ids=_id)
def test_scan_full_lengths_equal_the_plain_call(ovr):
    """seq_lens = [L] * B against the same call without seq_lens (whatever
    kernel that takes): 1e-5 of the scale, the bound between the scan paths."""
    from mtts import _lib, ops
    B, D, L = 6, 70, 130
    g = torch.Generator(device=DEV).manual_seed(5)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    u, z, dl, Bm, Cm = r(B, L, D), r(B, L, D), r(B, L, D) * 0.5, r(B, L, 16), r(B, L, 16)
    A, Dp, bias, h0 = -torch.exp(r(D, 16) * 0.5), r(D), r(D) * 0.1, r(B, D, 16) * 0.5
    with _lib.override(**ovr):
        o0, l0, _ = ops.scan_fwd(u, dl, A, Bm, Cm, Dp, z, bias, True, h0=h0, want_last=True)
        o1, l1, _ = ops.scan_fwd(u, dl, A, Bm, Cm, Dp, z, bias, True, h0=h0, want_last=True,
                                 seq_lens=torch.full((B,), L, dtype=torch.int32, device=DEV))
        o2, l2, _ = ops.scan_fwd(u, dl, A, Bm, Cm, Dp, z, bias, True, h0=h0, want_last=True, seq_lens=[L + 5] * B)
    for o, l in ((o1, l1), (o2, l2)):   # a length past L is clamped to L
        eo, so = _rel(o, o0)
        el, sl_ = _rel(l, l0)
        assert eo <= 1e-5 * so and el <= 1e-5 * sl_, (eo, so, el, sl_)


@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("with_state", [False, True], ids=["fresh", "state"])
def test_conv_state_at_row_length(with_state, io):
    from mtts import ops
    B, D, L, K = 6, 64, 9, 4
    lens = [9, 1, 2, 3, 5, 0]
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(B, L, D, device=DEV, generator=g).to(DT[io])
    w = torch.randn(D, K, device=DEV, generator=g)
    b = torch.randn(D, device=DEV, generator=g)
    st = torch.randn(B, D, K, device=DEV, generator=g) if with_state else None
    out0, st0 = ops.conv_fwd(x, w, b, True, state_in=st, want_state=True)
    for sl in (torch.tensor(lens, dtype=torch.int32, device=DEV), lens):
        out1, st1 = ops.conv_fwd(x, w, b, True, state_in=st, want_state=True, seq_lens=sl)
        assert torch.equal(out1, out0)                                # the convolution itself is untouched
        prev = st if with_state else torch.zeros(B, D, K, device=DEV)
        for r, n in enumerate(lens):
            want = torch.cat([prev[r], x[r, :n].float().transpose(0, 1)], dim=-1)[:, -K:]
            assert torch.equal(st1[r], want), (r, n)                  # a copy: exact
    full, stf = ops.conv_fwd(x, w, b, True, state_in=st, want_state=True, seq_lens=[L] * B)
    assert torch.equal(stf, st0) and torch.equal(full, out0)


def _embed_at(tok, pos, tw, pw, dtype, pos_bs, n_pos=None, entry="mtts_embed_sum_at"):
    from mtts import _lib
    from mtts.embed import _err_flag
    B, Ln = tok.shape
    d = tw.shape[1]
    qw = torch.randn(1, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    qid = torch.zeros(Ln, dtype=torch.int32, device=DEV)
    out = torch.full((B, Ln, d), 3.0, device=DEV, dtype=dtype)
    flag = _err_flag(tok.device)
    flag.zero_()
    args = [tok.data_ptr(), tok.stride(0), qid.data_ptr(), pos.data_ptr(), tw.data_ptr(), qw.data_ptr(), pw.data_ptr(),
            B, Ln, d, tw.shape[0], out.data_ptr(), _lib.dtype_code(out), out.stride(0), flag.data_ptr()]
    if entry == "mtts_embed_sum_at":
        args += [pos_bs, pw.shape[0] if n_pos is None else n_pos]
    _lib.call_raw(entry, *args)
    flagged = int(flag.item())
    flag.zero_()
    return out, qw, flagged


@pytest.mark.parametrize("Ln", [1, 5])
def test_embed_sum_at_per_row_positions(Ln):
    B, d, V, NP = 4, 64, 10, 50
    g = torch.Generator(device=DEV).manual_seed(Ln)
    tw, pw = torch.randn(V, d, device=DEV, generator=g), torch.randn(NP, d, device=DEV, generator=g)
    tok = torch.randint(0, V, (B, Ln), device=DEV, generator=g)
    pos = torch.randint(0, NP, (B, Ln), device=DEV, generator=g).to(torch.int32)
    pos[0, 0], pos[B - 1, Ln - 1] = 0, NP - 1                          # both ends of the table
    out, qw, flagged = _embed_at(tok, pos, tw, pw, torch.float32, pos.stride(0))
    want = (tw[tok] + pw[pos.long()]) + qw[0]
    assert not flagged and torch.equal(out, want)
    out16, _, flagged = _embed_at(tok, pos, tw, pw, torch.bfloat16, pos.stride(0))
    assert not flagged and torch.equal(out16, want.to(torch.bfloat16))  # round to nearest even of the fp32 sum
    # a position outside [0, n_pos): flagged, a zero row, the other rows as before
    for bad in (NP, -1):
        p2 = pos.clone()
        p2[1, Ln - 1] = bad
        o2, _, flagged = _embed_at(tok, p2, tw, pw, torch.float32, p2.stride(0))
        w2 = want.clone()
        w2[1, Ln - 1] = 0.0
        assert flagged == 1 and torch.equal(o2, w2), bad
    # n_pos is the caller's bound, not the table's: a shorter bound flags what lies past it
    o3, _, flagged = _embed_at(tok, pos, tw, pw, torch.float32, pos.stride(0), n_pos=NP - 1)
    assert flagged == 1 and (o3[B - 1, Ln - 1] == 0).all()
    # pos_bs = 0: one (L,) row shared by the batch, bitwise the old entry point
    shared = pos[2].contiguous()
    a, _, _ = _embed_at(tok, shared, tw, pw, torch.float32, 0)
    b, _, _ = _embed_at(tok, shared, tw, pw, torch.float32, 0, entry="mtts_embed_sum")
    assert torch.equal(a, b) and torch.equal(a, (tw[tok] + pw[shared.long()][None]) + qw[0])


def test_sampler_advances_per_row_positions():
    from mtts import ops
    B, V = 5, 64
    logits = torch.randn(B, V, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    start = torch.tensor([7, 0, 3, 100, 1], dtype=torch.int32, device=DEV)
    pos = start.clone()
    fin = torch.tensor([0, 1, 0, 0, 1], dtype=torch.int32, device=DEV)   # finished rows move too: lockstep
    for _ in range(3):
        ops.sample_tokens(logits, temperature=0.0, seed=0, step=step, advance=True, pos=pos, finished=fin)
    assert torch.equal(pos, start + 3) and int(step) == 3
    # a one-element pos: only that counter moves
    pos = start.clone()
    for _ in range(3):
        ops.sample_tokens(logits, temperature=0.0, seed=0, step=step, advance=True, pos=pos[2:3])
    assert pos.tolist() == [7, 0, 6, 100, 1] and int(step) == 6
    # without advance nothing moves
    ops.sample_tokens(logits, temperature=0.0, seed=0, step=step, advance=False, pos=pos)
    assert pos.tolist() == [7, 0, 6, 100, 1] and int(step) == 6
    with pytest.raises(ValueError):
        ops.sample_tokens(logits, temperature=0.0, seed=0, step=step, advance=True, pos=pos[:3])
