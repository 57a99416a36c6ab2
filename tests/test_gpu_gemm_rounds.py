"""mtts_gemm_grouped_rounds (csrc/gemm.hip): the grouped TN weight-gradient
launch with up to 64 problems and a tile grid larger than the CU count.

One call with 30 problems -- more than mtts_gemm_grouped's 24 -- against the
same problems run through mtts_gemm_grouped in chunks (the same tile body:
bit-equal) and against fp32 products of the same bf16 operands (rel < 1e-5,
test_gpu_gemm.py's bound for fp32 weight gradients).

Shapes.  24 of the problems cycle through (m, n) = 256x256, 512x256, 264x520,
96x512, 256x64, 8x8 with K from 64 / 128 / 1024, beta 0 and 1, some outputs
row slices of one buffer.  Those are at most 6 tiles each (52 in all), fewer
than a device's CUs, and the launch is only interesting when a CU runs more
than one workgroup and the last round's XCD renumbering takes its remainder
branch; so 6 further problems of 1032x2064 (5 x 9 ragged tiles, K 64 / 128)
bring the grid to 322 tiles: above 256 (and 304) CUs and 2 modulo 8.  The
test asserts both properties for the device it runs on."""
import ctypes

import pytest
import torch

from mtts import _lib as L
from mtts import gemm as G

pytestmark = pytest.mark.gpu
dev = "cuda"

SMALL = [(256, 256), (512, 256), (264, 520), (96, 512), (256, 64), (8, 8)]
KS = [64, 128, 1024]
BIG = (1032, 2064)


def rnd(*s, scale=0.5):
    return ((torch.rand(*s, device=dev) * 2 - 1) * scale).to(torch.bfloat16)


def rel(x, ref):
    return ((x.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-30)).item()


def _args(probs):
    arr = (L.GemmArgs * max(len(probs), 1))()
    for a, (dy, x, out, beta) in zip(arr, probs):
        a.m, a.n, a.k, a.layout, a.splits, a.out_dtype = dy.shape[1], x.shape[1], dy.shape[0], G.TN, 1, 0
        a.lda, a.ldb, a.ldc = dy.stride(0), x.stride(0), out.stride(0)
        a.a, a.b, a.c, a.beta = dy.data_ptr(), x.data_ptr(), out.data_ptr(), beta
    return arr


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rounds(probs, n=None, arr=None):
    arr = _args(probs) if arr is None else arr
    return L.lib().mtts_gemm_grouped_rounds(arr, len(probs) if n is None else n, _stream())


def _grouped_chunks(probs):
    for s in range(0, len(probs), 24):
        chunk = probs[s:s + 24]
        assert L.lib().mtts_gemm_grouped(_args(chunk), len(chunk), _stream()) == 0


def _tiles(probs):
    return sum(-(-dy.shape[1] // 256) * -(-x.shape[1] // 256) for dy, x, _, _ in probs)


@pytest.fixture(scope="module")
def problems():
    """30 (dy, x, initial output, beta, row slice of the shared buffer | None),
    longest K first; never written to."""
    torch.manual_seed(21)
    specs = [(SMALL[i % 6], KS[(i + i // 6) % 3], float(i % 2)) for i in range(24)]
    specs += [(BIG, KS[i % 2], float(i % 2)) for i in range(6)]
    shared = torch.randn(256 + 512 + 256, 256, device=dev)     # three row-slice outputs
    slices = {0: (0, 256), 1: (256, 768), 6: (768, 1024)}       # problems 0, 1, 6: 256 / 512 / 256 rows x 256
    out = []
    for i, ((m, n), k, beta) in enumerate(specs):
        dy, x = rnd(k, m), rnd(k, n)
        if i in slices:
            init = None
        elif beta:
            init = torch.randn(m, n, device=dev)
        else:
            init = torch.full((m, n), float("nan"), device=dev)
        out.append((dy, x, init, beta, slices.get(i)))
    out.sort(key=lambda t: -t[0].shape[0])
    return shared, out


def _materialise(problems):
    """Fresh outputs (clones of the initial values) for one run."""
    shared, specs = problems
    buf = shared.clone()
    probs = []
    for dy, x, init, beta, sl in specs:
        o = buf[sl[0]:sl[1]] if sl is not None else init.clone()
        probs.append((dy, x, o, beta))
    return buf, probs


def _expected(problems):
    shared, specs = problems
    refs = []
    for dy, x, init, beta, sl in specs:
        prod = dy.float().t() @ x.float()
        base = shared[sl[0]:sl[1]] if sl is not None else init
        refs.append(prod + base if beta else prod)
    return refs


def test_rounds_30_problems_equal_grouped_chunks_and_fp32(problems):
    buf_r, probs_r = _materialise(problems)
    buf_g, probs_g = _materialise(problems)
    assert len(probs_r) == 30
    tiles = _tiles(probs_r)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles > cus and tiles % 8 != 0, (tiles, cus)
    assert _rounds(probs_r) == 0, L.lib().mtts_last_error().decode()
    _grouped_chunks(probs_g)
    refs = _expected(problems)
    for i, ((_, _, o_r, _), (_, _, o_g, _), ref) in enumerate(zip(probs_r, probs_g, refs)):
        assert torch.isfinite(o_r).all(), i
        assert torch.equal(o_r, o_g), i
        assert rel(o_r, ref) < 1e-5, (i, rel(o_r, ref))
    assert torch.equal(buf_r, buf_g)


def test_rounds_rejects_bad_calls():
    lib = L.lib()
    dy, x = rnd(128, 256), rnd(128, 256)
    out = torch.empty(256, 256, device=dev)

    def refused(rc):
        return rc != 0 and len(lib.mtts_last_error()) > 0

    assert refused(_rounds([(dy, x, out, 0.0)], n=0))                      # no problems
    assert refused(_rounds([(dy, x, out, 0.0)] * 65))                      # above the 64-problem limit
    assert refused(_rounds([(dy, x, out, 0.5)]))                           # beta must be 0 or 1
    assert refused(_rounds([(rnd(100, 256), rnd(100, 256), out, 0.0)]))    # k % 64
    arr = _args([(dy, x, out, 0.0)])
    arr[0].a = None
    assert refused(_rounds([(dy, x, out, 0.0)], arr=arr))                  # null pointer
    assert refused(lib.mtts_gemm_grouped_rounds(None, 1, _stream()))
    assert _rounds([(dy, x, out, 0.0)] * 64) == 0                          # the limit itself is accepted
    torch.cuda.synchronize()


def test_rounds_deterministic(problems):
    runs = []
    for _ in range(2):
        buf, probs = _materialise(problems)
        assert _rounds(probs) == 0
        runs.append((buf, [o for _, _, o, _ in probs]))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
