"""CPU-side checks of the token sampler's boundary and of its float64
reference (tests/sample_ref.py): MttsSampleArgs as the C compiler lays it out
against the ctypes mirror, the exported symbol and ABI version, and the
reference sampler against the distributions it must draw from -- checked on
its own, so that kernel and reference cannot be wrong in the same way."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

import sample_ref as SR

HEADER = os.path.join(ROOT, "include", "mtts.h")
LOGITS = np.array([2, 1, .5, 0, -.5, -1, .3, 1.5, -2, .1])
ROWS = 20000
CHI2_BOUND = 33.7   # the issue's bound (chi-square, 9 degrees of freedom, p = 1e-4)


def test_sample_args_layout_symbol_and_abi():
    from mtts import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(MttsSampleArgs));']
    for fname, _ in _lib.SampleArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(MttsSampleArgs, {fname}));')
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
        got = ctypes.sizeof(_lib.SampleArgs) if field == "size" else getattr(_lib.SampleArgs, field).offset
        assert got == int(val), f"SampleArgs.{field}: ctypes {got} != C {val}"
        seen += 1
    assert seen == len(_lib.SampleArgs._fields_) + 1
    lib = _lib.lib()
    assert hasattr(lib, "mtts_sample_tokens") and "mtts_sample_tokens" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 15 and lib.mtts_abi_version() == 15


def _chi2(tokens, p):
    n = len(tokens)
    obs = np.bincount(tokens, minlength=len(p)).astype(np.float64)
    sel = p > 0
    assert obs[~sel].sum() == 0
    return float((((obs[sel] - n * p[sel]) ** 2) / (n * p[sel])).sum())


def _draw(step, **kw):
    return SR.sample_ref(np.tile(LOGITS, (ROWS, 1)), seed=99, step=step, **kw)[0]


def test_reference_draws_from_softmax():
    p = np.exp(LOGITS) / np.exp(LOGITS).sum()
    t0 = _draw(0, temperature=1.0)
    chi = _chi2(t0, p)
    print(f"chi-square vs softmax, 9 dof: {chi:.2f}")
    assert chi < CHI2_BOUND, chi
    # a new step draws new numbers: rows agree about sum p^2 (21 %) of the time
    for step in (1, 2):
        agree = float((_draw(step, temperature=1.0) == t0).mean())
        print(f"step {step} agrees with step 0 on {agree:.3f} of the rows (sum p^2 = {(p * p).sum():.3f})")
        assert abs(agree - (p * p).sum()) < 0.03, agree


def test_reference_top_k_top_p_kept_set():
    # top_k = 3 keeps logits {2, 1.5, 1}; of their softmax (.5065, .3072, .1863) the
    # third has S_> = .8137 >= .8 and leaves: tokens 0 and 7 remain
    t = _draw(0, temperature=1.0, top_k=3, top_p=0.8)
    assert set(np.unique(t).tolist()) <= {0, 7}
    p = np.zeros(10)
    p[[0, 7]] = np.exp(LOGITS[[0, 7]])
    p /= p.sum()
    chi = _chi2(t, p)
    print(f"chi-square vs the renormalised kept set: {chi:.2f}")
    assert chi < CHI2_BOUND, chi


def test_reference_greedy_ties_and_empty_rows():
    x = np.array([[1.0, 3.0, 3.0, -np.inf], [-np.inf] * 4, [np.nan, -1.0, np.nan, -np.inf]])
    tok, acc = SR.sample_ref(x, temperature=0.0, pad_id=2)
    assert tok.tolist() == [1, 2, 1] and acc == [{1}, {2}, {1}]
    tok, acc = SR.sample_ref(x, temperature=1.0, top_k=1, seed=5, step=3, pad_id=2)
    assert tok[1] == 2 and tok[2] == 1 and tok[0] in (1, 2)          # the tie at the top-k threshold keeps both
    exact, k_in, k_out = SR.kept_sets(x[0], 1.0, 1, 1.0)
    assert exact.tolist() == [False, True, True, False]
    # top_p tiny: only the most likely token(s) survive, and always do
    exact, k_in, k_out = SR.kept_sets(np.array([0.0, 2.0, 1.0]), 1.0, 0, 1e-6)
    assert exact.tolist() == [False, True, False] and k_out.tolist() == [False, True, False]
