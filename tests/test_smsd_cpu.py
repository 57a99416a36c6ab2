"""CPU-side checks of the SMSD mixture-density head: the drop-in module's
interface (state-dict keys and shapes against the list recorded from the
reference, no `transformers` import), the C ABI of csrc/mdn.hip (symbols,
struct layouts, argument checks that need no device), and the float64
restatement tests/smsd_ref.py on its own: against every value recorded from
the reference in tests/golden/smsd.npz, and its generators against the
distributions they must draw from."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import smsd_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mtts.h")
SYMBOLS = ("mtts_mdn_params_fwd", "mtts_mdn_params_bwd", "mtts_mixture_nll_fwd", "mtts_mixture_nll_bwd",
           "mtts_mixture_sample", "mtts_relu_dropout", "mtts_mdn_layernorm_fwd", "mtts_mdn_layernorm_bwd")
STRUCTS = {"MttsMdnParamsArgs": "MdnParamsArgs", "MttsMdnParamsBwdArgs": "MdnParamsBwdArgs",
           "MttsMixtureNllArgs": "MixtureNllArgs", "MttsMixtureNllBwdArgs": "MixtureNllBwdArgs",
           "MttsMixtureSampleArgs": "MixtureSampleArgs", "MttsReluDropoutArgs": "ReluDropoutArgs",
           "MttsRowLNArgs": "RowLNArgs", "MttsRowLNBwdArgs": "RowLNBwdArgs"}
EINVAL = -22


# ---- the module's interface -----------------------------------------------------

def test_import_smsd_does_not_import_transformers():
    code = ("import sys; sys.path[:0] = [%r, %r]; import smsd; "
            "assert 'transformers' not in sys.modules, 'transformers imported'; "
            "m = smsd.SMSD(bert_model=None, bert_dim=24, style_dim=8, num_mixtures=3, hidden_dim=16); "
            "assert 'transformers' not in sys.modules; "
            "assert all(k.startswith('mdn_head.') for k in m.state_dict()); print('ok')"
            % (ROOT, os.path.join(ROOT, "mamba-tts-project_amd")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


@pytest.mark.parametrize("mode", R.MODES)
def test_state_dict_keys_and_shapes_match_the_reference(golden, mode):
    import smsd
    g = golden("smsd.npz")
    want = {k: tuple(int(n) for n in s.split(",") if n) for k, s in zip(g[f"{mode}/keys"].tolist(),
                                                                       g[f"{mode}/shapes"].tolist())}
    head = smsd.MDNHead(768, 256, 5, 512, variance_mode=mode)
    got = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    full = smsd.SMSD(bert_model=None, variance_mode=mode)     # the reference's defaults otherwise
    assert {k: tuple(v.shape) for k, v in full.state_dict().items()} == {"mdn_head." + k: s for k, s in want.items()}
    assert (full.style_dim, full.num_mixtures, full.variance_mode) == (256, 5, mode)


def test_default_mode_key_table():
    import smsd
    sd = smsd.MDNHead(768, 256, 5, 512).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "mlp.0.weight": (768,), "mlp.0.bias": (768,), "mlp.1.weight": (512, 768), "mlp.1.bias": (512,),
        "mlp.4.weight": (512, 512), "mlp.4.bias": (512,), "pi_head.weight": (5, 512), "pi_head.bias": (5,),
        "mu_head.weight": (1280, 512), "mu_head.bias": (1280,), "sigma_head.weight": (1, 512),
        "sigma_head.bias": (1,), "noise_net.noise_scale": ()}
    assert "sigma_head.weight" not in smsd.MDNHead(8, 4, 2, 8, variance_mode="fixed").state_dict()
    assert "noise_net.noise_scale" not in smsd.MDNHead(8, 4, 2, 8, variance_mode="fixed").state_dict()


def test_strings_need_an_encoder_and_cpu_tensors_raise():
    import smsd
    m = smsd.SMSD(bert_model=None, bert_dim=24, style_dim=8, num_mixtures=3, hidden_dim=16)
    with pytest.raises(TypeError, match="bert_model=None"):
        m(["speak slowly"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 24))
    with pytest.raises(RuntimeError, match="no CPU path"):
        smsd.mixture_nll_loss(torch.zeros(2, 8), torch.full((2, 3), 1 / 3), torch.zeros(2, 3, 8), torch.ones(2))
    with pytest.raises(ValueError, match="variance_mode"):
        smsd.MDNHead(8, 4, 2, 8, variance_mode="full")


# ---- the C ABI ------------------------------------------------------------------

def test_library_exports_the_symbols_and_the_versions_agree():
    from mtts import _lib
    lib = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s), f"libmtts.so does not export {s}"
        assert s in _lib.exported_symbols()
    assert lib.mtts_abi_version() == _lib.ABI_VERSION


def test_struct_layouts_match_the_header():
    from mtts import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("maxk - %d\\n", MTTS_MDN_MAX_K);',
             'printf("modes - %d\\n", MTTS_MDN_SHARED + 10 * MTTS_MDN_ISOTROPIC + 100 * MTTS_MDN_DIAGONAL + 1000 * MTTS_MDN_FIXED);',
             'printf("noise - %d\\n", MTTS_MDN_NOISE_NONE + 10 * MTTS_MDN_NOISE_GIVEN + 100 * MTTS_MDN_NOISE_DRAWN);']
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'printf("{pyname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    consts = {}
    for line in out.strip().splitlines():
        py, field, val = line.split()
        if field == "-":
            consts[py] = int(val)
            continue
        cls = getattr(_lib, py)
        got = C.sizeof(cls) if field == "size" else getattr(cls, field).offset
        assert got == int(val), f"{py}.{field}: ctypes {got} != C {val}"
    m = _lib.MDN_MODES
    assert consts["maxk"] == _lib.MDN_MAX_K == 32
    assert consts["modes"] == (m["isotropic_across_clusters"] + 10 * m["isotropic"] + 100 * m["diagonal"]
                               + 1000 * m["fixed"])
    assert consts["noise"] == _lib.MDN_NOISE_NONE + 10 * _lib.MDN_NOISE_GIVEN + 100 * _lib.MDN_NOISE_DRAWN


# Every check of an entry point runs before its first HIP call, so a struct
# that fails one returns MTTS_EINVAL without a device.  Every row below MUST
# fail a check: PTR is a host address that no kernel may ever see.
_BUF = (C.c_char * 64)()
PTR = C.addressof(_BUF)


def _params(**kw):
    from mtts import _lib
    a = _lib.MdnParamsArgs()
    a.rows, a.K, a.d, a.mode, a.dtype, a.noise = 2, 5, 8, 0, 0, 0
    a.logits_rs = a.pi_rs = 5
    a.sraw_rs = a.sigma_rs = a.eps_rs = 1
    a.pi_logits = a.sigma_raw = a.pi = a.sigma = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _nll(**kw):
    from mtts import _lib
    a = _lib.MixtureNllArgs()
    a.rows, a.K, a.d, a.mode, a.dtype = 2, 5, 8, 0, 0
    a.y_rs, a.pi_rs, a.mu_rs, a.sigma_rs = 8, 5, 40, 1
    a.y = a.pi = a.mu = a.sigma = a.loss = a.lse = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _sample(**kw):
    from mtts import _lib
    a = _lib.MixtureSampleArgs()
    a.rows, a.K, a.d, a.mode, a.dtype = 2, 5, 8, 0, 0
    a.pi_rs, a.mu_rs, a.sigma_rs, a.out_rs = 5, 40, 1, 8
    a.pi = a.mu = a.sigma = a.seed = a.out = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _relu(**kw):
    from mtts import _lib
    a = _lib.ReluDropoutArgs()
    a.n, a.dtype, a.p = 8, 0, 0.1
    a.x = a.out = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rowln(**kw):
    from mtts import _lib
    a = _lib.RowLNArgs()
    a.rows, a.cols, a.dtype, a.eps, a.x_rs, a.y_rs = 2, 24, 0, 1e-5, 24, 24
    a.x = a.w = a.b = a.y = a.mean = a.rstd = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd(cls_name, f):
    from mtts import _lib
    g = getattr(_lib, cls_name)()
    g.f = f
    return g


BAD = [
    ("mtts_mdn_params_fwd", lambda: _params(K=0), "K=0"),
    ("mtts_mdn_params_fwd", lambda: _params(K=33), "K=33"),
    ("mtts_mdn_params_fwd", lambda: _params(mode=4), "unknown variance mode"),
    ("mtts_mdn_params_fwd", lambda: _params(mode=-1), "unknown variance mode"),
    ("mtts_mdn_params_fwd", lambda: _params(dtype=2), "dtype"),
    ("mtts_mdn_params_fwd", lambda: _params(pi=None), "null pointer"),
    ("mtts_mdn_params_fwd", lambda: _params(sigma_raw=None), "sigma_raw"),
    ("mtts_mdn_params_fwd", lambda: _params(sigma=None), "null sigma"),
    ("mtts_mdn_params_fwd", lambda: _params(pi_rs=4), "row strides below K"),
    ("mtts_mdn_params_fwd", lambda: _params(mode=1), "sigma_raw"),                       # stride 1 < K
    ("mtts_mdn_params_fwd", lambda: _params(mode=2, sraw_rs=40, sigma_rs=39), "sigma row stride"),
    ("mtts_mdn_params_fwd", lambda: _params(noise=3), "unknown noise kind"),
    ("mtts_mdn_params_fwd", lambda: _params(noise=1, noise_scale=PTR), "eps"),
    ("mtts_mdn_params_fwd", lambda: _params(noise=2, noise_scale=PTR), "row seeds"),
    ("mtts_mdn_params_fwd", lambda: _params(noise=1, eps=PTR), "noise_scale"),
    ("mtts_mdn_params_fwd", lambda: _params(mode=3, noise=1), "fixed mode"),
    ("mtts_mdn_params_bwd", lambda: _bwd("MdnParamsBwdArgs", _params()), "null pi gradient"),
    ("mtts_mdn_params_bwd", lambda: _bwd("MdnParamsBwdArgs", _params(K=33)), "K=33"),
    ("mtts_mixture_nll_fwd", lambda: _nll(K=0), "K=0"),
    ("mtts_mixture_nll_fwd", lambda: _nll(K=33), "K=33"),
    ("mtts_mixture_nll_fwd", lambda: _nll(mode=7), "unknown variance mode"),
    ("mtts_mixture_nll_fwd", lambda: _nll(mu=None), "null pointer"),
    ("mtts_mixture_nll_fwd", lambda: _nll(lse=None), "null pointer"),
    ("mtts_mixture_nll_fwd", lambda: _nll(sigma=None), "null sigma"),
    ("mtts_mixture_nll_fwd", lambda: _nll(mode=1), "sigma row stride"),
    ("mtts_mixture_nll_fwd", lambda: _nll(mode=2, sigma_rs=39), "sigma row stride"),
    ("mtts_mixture_nll_fwd", lambda: _nll(mu_rs=39), "row stride is too short"),
    ("mtts_mixture_nll_fwd", lambda: _nll(dtype=-1), "dtype"),
    ("mtts_mixture_nll_fwd", lambda: _nll(rows=0), "must be positive"),
    ("mtts_mixture_nll_bwd", lambda: _bwd("MixtureNllBwdArgs", _nll()), "null gradient pointer"),
    ("mtts_mixture_nll_bwd", lambda: _bwd("MixtureNllBwdArgs", _nll(K=0)), "K=0"),
    ("mtts_mixture_sample", lambda: _sample(K=0), "K=0"),
    ("mtts_mixture_sample", lambda: _sample(K=33), "K=33"),
    ("mtts_mixture_sample", lambda: _sample(mode=4), "unknown variance mode"),
    ("mtts_mixture_sample", lambda: _sample(seed=None), "null pointer"),
    ("mtts_mixture_sample", lambda: _sample(sigma=None), "null sigma"),
    ("mtts_mixture_sample", lambda: _sample(out_rs=7), "row stride is too short"),
    ("mtts_mixture_sample", lambda: _sample(mode=1), "sigma row stride"),
    ("mtts_relu_dropout", lambda: _relu(x=None), "null pointer"),
    ("mtts_relu_dropout", lambda: _relu(dtype=3), "dtype"),
    ("mtts_relu_dropout", lambda: _relu(p=1.0), "must be in [0, 1)"),
    ("mtts_relu_dropout", lambda: _relu(n=-8), "must not be negative"),
    ("mtts_relu_dropout", lambda: _relu(x=PTR + 4), "16-byte aligned"),
    ("mtts_mdn_layernorm_fwd", lambda: _rowln(w=None), "null pointer"),
    ("mtts_mdn_layernorm_fwd", lambda: _rowln(cols=0), "must be positive"),
    ("mtts_mdn_layernorm_fwd", lambda: _rowln(dtype=2), "dtype"),
    ("mtts_mdn_layernorm_fwd", lambda: _rowln(y_rs=23), "row stride is below cols"),
    ("mtts_mdn_layernorm_bwd", lambda: _bwd("RowLNBwdArgs", _rowln()), "null gradient pointer"),
    ("mtts_mdn_layernorm_bwd", lambda: _bwd("RowLNBwdArgs", _rowln(rows=0)), "must be positive"),
]


@pytest.mark.parametrize("row", BAD, ids=[f"{e}-{m.replace(' ', '_')}-{i}" for i, (e, _, m) in enumerate(BAD)])
def test_entry_points_refuse_invalid_arguments(row):
    from mtts import _lib
    entry, make, message = row
    lib = _lib.lib()
    rc = getattr(lib, entry)(C.byref(make()), None)
    assert rc == EINVAL
    assert message in lib.mtts_last_error().decode()


@pytest.mark.parametrize("entry", SYMBOLS)
def test_entry_points_refuse_a_null_struct(entry):
    from mtts import _lib
    lib = _lib.lib()
    assert getattr(lib, entry)(None, None) == EINVAL
    assert "null pointer" in lib.mtts_last_error().decode()


# ---- the restatement against the reference's recorded values -------------------------

def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.max(np.abs(got - want)) if got.size else 0.0
    assert err <= 1e-12 * max(1.0, np.max(np.abs(want))), f"{what}: {err}"


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_reproduces_every_recorded_value(golden, mode):
    g = golden("smsd.npz")
    sd = {k[len(mode) + 4:]: _t(v) for k, v in g.items() if k.startswith(f"{mode}/sd/")}
    x, y = _t(g[f"{mode}/x"]), _t(g[f"{mode}/y"])
    pi, mu, sigma = R.head(sd, x, mode, 5, 40)
    _close(pi, g[f"{mode}/pi"], "pi")
    _close(mu, g[f"{mode}/mu"], "mu")
    _close(sigma, g[f"{mode}/sigma"], "sigma")
    if mode != "fixed":
        sraw, eps = _t(g[f"{mode}/noise_in"]), _t(g[f"{mode}/noise_eps"])
        _close(sraw + sd["noise_net.noise_scale"] * eps, g[f"{mode}/noise_out"], "NoiseNet")
        _, s_train = R.params(torch.zeros(3, 5, dtype=torch.float64), sraw, mode, 5, 40, sd["noise_net.noise_scale"], eps)
        _close(s_train, torch.nn.functional.softplus(_t(g[f"{mode}/noise_out"])).reshape(s_train.shape), "sigma (training)")
        _, _, s_head = R.head(sd, x, mode, 5, 40, epsilon=eps)
        _close(s_head, s_train, "sigma (training, through the head)")
    Bl = g[f"{mode}/g_y"].shape[0]
    assert Bl == (1 if mode == "isotropic_across_clusters" else 3)
    loss, gy, gpi, gmu, gs = R.nll_and_grads(y[:Bl], pi[:Bl], mu[:Bl], sigma[:Bl], mode)
    _close(loss, g[f"{mode}/loss"], "loss")
    _close(gy, g[f"{mode}/g_y"], "g_y")
    _close(gpi, g[f"{mode}/g_pi"], "g_pi")
    _close(gmu, g[f"{mode}/g_mu"], "g_mu")
    if mode == "fixed":
        assert gs is None and f"{mode}/g_sigma" not in g
    else:
        _close(gs, g[f"{mode}/g_sigma"], "g_sigma")


def test_fixture_is_float64_and_small(golden):
    g = golden("smsd.npz")
    for k, v in g.items():
        assert v.dtype == np.float64 or k.endswith(("/keys", "/shapes")), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "smsd.npz")) < 512 * 1024


def test_default_mode_uses_each_rows_own_variance():
    """The documented formula at B == K and at a B where the reference raises:
    the batch loss is the mean of the rows' own losses."""
    torch.manual_seed(3)
    for B in (5, 3):
        K, d = 5, 6
        y, mu = torch.randn(B, d, dtype=torch.float64), torch.randn(B, K, d, dtype=torch.float64)
        pi = torch.softmax(torch.randn(B, K, dtype=torch.float64), -1)
        sigma = torch.rand(B, dtype=torch.float64) + 0.5
        whole = R.mixture_nll(y, pi, mu, sigma, "isotropic_across_clusters")
        rows = [R.mixture_nll(y[b:b + 1], pi[b:b + 1], mu[b:b + 1], sigma[b:b + 1], "isotropic_across_clusters")
                for b in range(B)]
        assert abs(whole - torch.stack(rows).mean()) < 1e-12
        same = R.mixture_nll(y, pi, mu, sigma[:, None].expand(B, K), "isotropic")
        assert abs(whole - same) < 1e-12


# ---- the generators ---------------------------------------------------------------

def test_normal_generator_moments():
    N = 1 << 18
    z = R.normals(R.stream_key(1234, 7), N)
    assert z.shape == (N,)
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2 / N)
    assert np.abs(z).max() <= 5.9
    e = R.normals(R.stream_key(1234, 0), N, R.TAG_EPS)
    assert abs(e.mean()) <= 5 / np.sqrt(N) and abs(e.var() - 1.0) <= 5 * np.sqrt(2 / N)
    assert not np.array_equal(e[:64], R.normals(R.stream_key(1234, 0), 64))      # the streams differ
    assert np.array_equal(R.normals(R.stream_key(1234, 7), 33), z[:33])           # a prefix does not depend on n


def test_categorical_draw_frequencies():
    N = 20000
    pi = np.array([0.05, 0.3, 0.15, 0.4, 0.1], dtype=np.float32)
    seeds = R.row_seeds(99, N)
    ks = np.array([R.pick(pi, R.stream_key(s))[0] for s in seeds])
    p = pi.astype(np.float64) / pi.astype(np.float64).sum()
    freq = np.bincount(ks, minlength=5) / N
    assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)), (freq, p)
    # the draw count moves the stream; one seed, one draw count: one pick
    assert R.pick(pi, R.stream_key(5, 3)) == R.pick(pi, R.stream_key(5, 3))
    ks2 = np.array([R.pick(pi, R.stream_key(7, t))[0] for t in range(2000)])
    assert len(set(ks2.tolist())) == 5
    assert R.pick(np.array([1.0], dtype=np.float32), R.stream_key(1))[0] == 0
