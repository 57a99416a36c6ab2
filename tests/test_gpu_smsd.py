"""The SMSD mixture-density head on the GPU (csrc/mdn.hip through mtts.mdn and
the drop-in smsd.py) against the float64 restatement tests/smsd_ref.py, which
tests/test_smsd_cpu.py pins to the reference's recorded values.

Bounds.  fp32: per tensor max|err| <= 1e-3 max|ref| (the project's standing
fp32 bound; the reference in fp32 sits at 1.6e-7 / 1.4e-5 of it).  bf16: the
float64 result on the bf16-rounded inputs is the reference; scalar fp32
outputs keep 1e-3, bf16 tensors get 1e-3 + 2^-8 of the tensor's largest
magnitude (one bf16 rounding).  Sampler: component indices exact (on inputs
whose uniforms stay 2^-20 away from every CDF boundary, asserted), the noise
within 2e-5 absolute of the float64 Box-Muller of the same uniforms (fp32
logf / sincosf at a few ulp on |z| <= 5.9 give about 3e-6)."""
import numpy as np
import pytest
import torch

import smsd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(1, 5, 256), (3, 5, 256), (5, 5, 40), (2, 1, 8), (3, 7, 1000), (2, 32, 72)]
BF16_ULP = 2.0 ** -8


def check(got, ref, name, bf16_tensor=False, rtol=1e-3):
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(ref).detach().double().cpu().reshape(got.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite"
    scale = ref.abs().max().item() if ref.numel() else 0.0
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    bound = (rtol + (BF16_ULP if bf16_tensor else 0.0)) * scale
    print(f"{name}: max|err|={err:.3e} max|ref|={scale:.3e} bound={bound:.3e}")
    assert err <= bound, f"{name}: max|err|={err:.3e} > {bound:.3e} (max|ref|={scale:.3e})"


def rounded(t, dtype):
    """fp32 CPU tensor -> (device tensor in dtype, float64 CPU copy of the rounded values)."""
    r = t.to(dtype)
    return r.to(DEV), r.double()


def mixture_inputs(B, K, d, mode, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, d, generator=g)
    pi = torch.softmax(torch.randn(B, K, generator=g), -1)
    mu = torch.randn(B, K, d, generator=g)
    sigma = 0.5 + torch.rand(R.sigma_shape(mode, B, K, d), generator=g)
    if mode == "fixed":
        sigma = torch.full((B,), 0.1)
    return y, pi, mu, sigma


def run_nll(y, pi, mu, sigma, mode, dtype):
    """The kernel's loss and gradients against the restatement on the same (rounded) inputs."""
    from mtts import mdn
    dev, ref = zip(*(rounded(t, dtype) for t in (y, pi, mu, sigma)))
    leaves = [t.requires_grad_(True) for t in dev]
    loss = mdn.mixture_nll(*leaves, mode)
    assert loss.dtype == F32 and loss.dim() == 0
    loss.backward()
    rl, ry, rpi, rmu, rs = R.nll_and_grads(*ref, mode)
    bf = dtype == BF16
    check(loss, rl, "loss")
    check(leaves[0].grad, ry, "d y", bf)
    check(leaves[1].grad, rpi, "d pi", bf)
    check(leaves[2].grad, rmu, "d mu", bf)
    if mode == "fixed":
        assert leaves[3].grad is None
    else:
        check(leaves[3].grad, rs, "d sigma", bf)
    return loss, leaves


# ---- loss kernel ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_mixture_nll_fwd_bwd(B, K, d, mode, dtype):
    run_nll(*mixture_inputs(B, K, d, mode, 7 + B + K + d), mode, dtype)


@pytest.mark.parametrize("mode", R.MODES)
def test_mixture_nll_matches_the_recorded_reference(golden, mode):
    from mtts import mdn
    g = golden("smsd.npz")
    Bl = g[f"{mode}/g_y"].shape[0]
    y, pi, mu, sigma = (torch.from_numpy(g[f"{mode}/{n}"][:Bl]).float().to(DEV).requires_grad_(True)
                        for n in ("y", "pi", "mu", "sigma"))
    loss = mdn.mixture_nll(y, pi, mu, sigma, mode)
    loss.backward()
    check(loss, g[f"{mode}/loss"], "loss")
    check(y.grad, g[f"{mode}/g_y"], "d y")
    check(pi.grad, g[f"{mode}/g_pi"], "d pi")
    check(mu.grad, g[f"{mode}/g_mu"], "d mu")
    if mode != "fixed":
        check(sigma.grad, g[f"{mode}/g_sigma"], "d sigma")


def fp32_reference_is_finite(y, pi, mu, sigma, mode):
    leaves = [t.detach().clone().float().requires_grad_(True) for t in (y, pi, mu, sigma)]
    loss = R.mixture_nll(*leaves, mode)
    loss.backward()
    return bool(torch.isfinite(loss)) and all(torch.isfinite(t.grad).all() for t in leaves if t.grad is not None)


@pytest.mark.parametrize("mode", R.MODES)
def test_mixture_nll_floor_decides_an_underflowed_components_gradient(mode):
    """A component with logit -100 (its weight underflows next to 1e-8) that
    is nevertheless a likely one for y: log(pi + 1e-8) and d pi = w r /
    (pi + 1e-8) are decided by the floor.  Through softmax -> loss, so the
    parameter kernel's backward sees the large d pi as well."""
    from mtts import mdn
    B, K, d = 3, 5, 40
    y, _, mu, sigma = mixture_inputs(B, K, d, mode, 21)
    g = torch.Generator().manual_seed(22)
    logits = torch.randn(B, K, generator=g)
    logits[:, 2] = -100.0
    # y on that component's mean, the means spread so far that it shares the rows with the others: with them
    # much farther every other responsibility vanishes and d logits is left at fp32's subnormal quantum times d pi
    s = 0.1 if mode == "fixed" else 1.0
    mu = mu * s * {"isotropic_across_clusters": 0.8, "isotropic": 0.8, "diagonal": 0.6, "fixed": 0.7}[mode]
    y = mu[:, 2] + 0.05 * s * torch.randn(B, d, generator=g)
    pi64 = torch.softmax(logits.double(), -1)
    assert (pi64[:, 2] < 1e-30).all()
    assert fp32_reference_is_finite(y, torch.softmax(logits, -1), mu, sigma, mode)
    lg = logits.to(DEV).requires_grad_(True)
    pi, _ = mdn.mdn_params(lg, None if mode == "fixed" else torch.zeros(B, R.sigma_raw_width(mode, K, d), device=DEV),
                           None, mode, d)
    pi.retain_grad()
    loss = mdn.mixture_nll(y.to(DEV), pi, mu.to(DEV), sigma.to(DEV), mode)
    loss.backward()
    l64 = logits.double().requires_grad_(True)
    p64 = torch.softmax(l64, -1)
    p64.retain_grad()
    ref = R.mixture_nll(y.double(), p64, mu.double(), sigma.double(), mode)
    ref.backward()
    check(loss, ref, "loss")
    check(pi.grad, p64.grad, "d pi")
    check(pi.grad[:, 2], p64.grad[:, 2], "d pi of the floored component")
    assert (p64.grad[:, 2].abs() > 1e5).all()          # -(1/B) r / 1e-8, r the component's share of the row
    assert l64.grad.abs().max() > 1e-2
    check(lg.grad, l64.grad, "d logits")


@pytest.mark.parametrize("mode", R.MODES)
def test_mixture_nll_far_targets(mode):
    """y at 1e2 sigma from every mean: every exponent is near -5000, so the
    logsumexp must not leave the row maximum.  The means are spread so that one
    component wins each row by more than 20 nats (asserted): the fp32 rounding
    of exponents of that size (5e-4) then cannot move the responsibilities."""
    B, K, d = 3, 5, 40
    g = torch.Generator().manual_seed(43)
    mu = torch.randn(B, K, d, generator=g)
    sigma = torch.ones(R.sigma_shape(mode, B, K, d))
    s = 0.1 if mode == "fixed" else 1.0
    if mode == "fixed":
        sigma, mu = torch.full((B,), 0.1), 0.1 * mu
    u = torch.randn(B, d, generator=g)
    y = mu.mean(1) + 100.0 * s * u / u.norm(dim=1, keepdim=True)
    pi = torch.softmax(torch.randn(B, K, generator=g), -1)
    dist = (y[:, None] - mu).norm(dim=-1) / s
    assert (dist > 95).all() and (dist < 105).all()
    lw = torch.log(pi.double() + 1e-8) - 0.5 * ((y[:, None] - mu).double() ** 2).sum(-1) / s ** 2
    top = lw.sort(dim=1, descending=True).values
    assert (top[:, 0] - top[:, 1] > 20).all()
    assert fp32_reference_is_finite(y, pi, mu, sigma, mode)
    loss, _ = run_nll(y, pi, mu, sigma, mode, F32)
    assert loss.item() > 4000


def test_mixture_nll_is_deterministic_and_row_independent():
    from mtts import mdn
    y, pi, mu, sigma = (t.to(DEV) for t in mixture_inputs(5, 7, 333, "diagonal", 5))

    def grads(rows):
        rows = torch.tensor(rows, device=DEV)
        leaves = [t[rows].clone().requires_grad_(True) for t in (y, pi, mu, sigma)]
        loss = mdn.mixture_nll(*leaves, "diagonal")
        loss.backward()
        return loss.detach(), [t.grad for t in leaves]
    l0, g0 = grads([0, 1, 2, 3, 4])
    l1, g1 = grads([0, 1, 2, 3, 4])
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    # row 2 beside row 0, and at the other index beside row 4: the same gradients (both batches scale by 1 / 2)
    _, ga = grads([2, 0])
    _, gb = grads([4, 2])
    assert all(torch.equal(a[0], b[1]) for a, b in zip(ga, gb))
    assert not torch.equal(ga[2][1], gb[2][0])


# ---- parameter kernel ---------------------------------------------------------------

def params_inputs(B, K, d, mode, seed):
    g = torch.Generator().manual_seed(seed)
    S = R.sigma_raw_width(mode, K, d)
    logits = 3.0 * torch.randn(B, K, generator=g)
    sraw = -10.0 + 35.0 * torch.rand(B, S, generator=g)          # [-10, 25]: both softplus branches
    if S:
        sraw.view(-1)[-1] = -10.0
        sraw.view(-1)[0] = 25.0
    eps = torch.randn(B, S, generator=g)
    wp, ws = torch.randn(B, K, generator=g), torch.randn(B, S, generator=g)
    return logits, sraw, eps, wp, ws


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("B,K,d", SHAPES)
def test_mdn_params_fwd_bwd(B, K, d, mode, dtype):
    from mtts import mdn
    logits, sraw, eps, wp, ws = params_inputs(B, K, d, mode, 3 + B + K + d)
    bf = dtype == BF16
    (lg, lg64), (sr, sr64), (ep, ep64), (wpd, wp64), (wsd, ws64) = (rounded(t, dtype) for t in (logits, sraw, eps, wp, ws))
    ns = torch.tensor(0.1, device=DEV, requires_grad=True)
    lg.requires_grad_(True)
    sr.requires_grad_(True)
    fixed = mode == "fixed"
    if not fixed:
        both = (sr64 + 0.1 * ep64)
        assert (both > 20).any() and ((both < 20).any() or both.numel() == 1)
    pi, sigma = mdn.mdn_params(lg, None if fixed else sr, None if fixed else ns, mode, d, training=True,
                               epsilon=None if fixed else ep)
    assert pi.shape == (B, K) and tuple(sigma.shape) == R.sigma_shape(mode, B, K, d) and pi.dtype == dtype
    l64, s64 = lg64.clone().requires_grad_(True), sr64.clone().requires_grad_(True)
    n64 = torch.tensor(0.1, dtype=torch.float32).double().requires_grad_(True)
    rpi, rsig = R.params(l64, s64, mode, K, d, n64, None if fixed else ep64)
    check(pi, rpi, "pi", bf)
    check(sigma, rsig, "sigma", bf)
    if fixed:
        (pi * wpd).sum().backward()
        (rpi * wp64).sum().backward()
        check(lg.grad, l64.grad, "d logits", bf)
        return
    ((pi.float() * wpd.float()).sum() + (sigma.reshape(B, -1).float() * wsd.float()).sum()).backward()
    ((rpi * wp64).sum() + (rsig.reshape(B, -1) * ws64).sum()).backward()
    check(lg.grad, l64.grad, "d logits", bf)
    check(sr.grad, s64.grad, "d sigma_raw", bf)
    check(ns.grad, n64.grad, "d noise_scale")
    assert ns.grad.dtype == F32 and ns.grad.shape == ()


@pytest.mark.parametrize("mode", R.MODES[:3])
def test_mdn_params_matches_the_recorded_noisenet(golden, mode):
    from mtts import mdn
    g = golden("smsd.npz")
    sraw, eps = (torch.from_numpy(g[f"{mode}/{n}"]).float().to(DEV) for n in ("noise_in", "noise_eps"))
    ns = torch.from_numpy(g[f"{mode}/sd/noise_net.noise_scale"]).float().to(DEV)
    _, sigma = mdn.mdn_params(torch.zeros(3, 5, device=DEV), sraw, ns, mode, 40, training=True, epsilon=eps)
    want = torch.nn.functional.softplus(torch.from_numpy(g[f"{mode}/noise_out"]))
    check(sigma, want, "sigma = softplus(NoiseNet(sigma_raw))")
    _, sigma_eval = mdn.mdn_params(torch.zeros(3, 5, device=DEV), sraw, ns, mode, 40, training=False, epsilon=eps)
    check(sigma_eval, torch.nn.functional.softplus(torch.from_numpy(g[f"{mode}/noise_in"])), "sigma in eval: no noise")


def test_mdn_params_drawn_noise_is_the_restatements():
    """eps drawn in the kernel: recover it from sigma_raw = 0, noise_scale = 1
    (sigma = softplus(eps)) and compare with the restatement's stream; the
    backward regenerates it (d noise_scale = sum dsigma sigmoid(eps) eps)."""
    from mtts import dropout as D, mdn
    B, K, d, mode = 3, 5, 37, "diagonal"
    S = K * d
    base = int(D.device_base(DEV).item())
    seeds = torch.tensor([11, -5, 2 ** 40 + 3], dtype=torch.int64, device=DEV)
    sraw = torch.zeros(B, S, device=DEV, requires_grad=True)
    ns = torch.tensor(1.0, device=DEV, requires_grad=True)
    _, sigma = mdn.mdn_params(torch.zeros(B, K, device=DEV), sraw, ns, mode, d, training=True, seed=seeds)
    eps = R.noise_eps([(int(s) + base) & R.M64 for s in seeds.tolist()], S)
    want = torch.nn.functional.softplus(torch.from_numpy(eps))
    got = sigma.detach().double().cpu().reshape(B, S)
    assert (got - want).abs().max().item() <= 2e-5
    sigma.sum().backward()
    e = torch.from_numpy(eps)
    check(ns.grad, (torch.sigmoid(e) * e).sum(), "d noise_scale (drawn eps)")
    _, again = mdn.mdn_params(torch.zeros(B, K, device=DEV), sraw, ns, mode, d, training=True, seed=seeds)
    assert torch.equal(again, sigma)


# ---- the head's any-width LayerNorm --------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(3, 24), (1, 3), (5, 100), (2, 1000), (4, 257)])
def test_layer_norm_rows(rows, cols, dtype):
    """Widths ln.hip does not take: below a wave, not a multiple of the thread
    count, one past it, and the narrowest with a gradient to compare (at one
    and two columns dx is zero up to cancellation, so it has no scale)."""
    from mtts import mdn
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, cols, generator=g) * 2 + 0.5
    w, b, dy = 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g), torch.randn(rows, cols, generator=g)
    (xd, x64), (dyd, dy64) = rounded(x, dtype), rounded(dy, dtype)
    xd.requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = mdn.layer_norm_rows(xd, wd, bd, 1e-5)
    assert y.dtype == dtype and y.shape == (rows, cols)
    y.backward(dyd)
    x64.requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(x64, (cols,), w64, b64, 1e-5)
    ref.backward(dy64)
    bf = dtype == BF16
    check(y, ref, "y", bf)
    check(xd.grad, x64.grad, "dx", bf)
    check(wd.grad, w64.grad, "dw")
    check(bd.grad, b64.grad, "db")


# ---- relu_dropout ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 1003, 4096])
def test_relu_dropout_p0_is_relu_bit_for_bit(n, dtype):
    from mtts import mdn
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV, dtype).requires_grad_(True)
    for training, p in ((True, 0.0), (False, 0.1)):
        y = mdn.relu_dropout(x, p, training)
        assert torch.equal(y, torch.relu(x))
        x.grad = None
        y.backward(torch.ones_like(y))
        assert torch.equal(x.grad, (x > 0).to(dtype))


def test_relu_dropout_mask():
    from mtts import dropout as D, mdn
    N, p = 1 << 20, 0.1
    x = (torch.rand(N, generator=torch.Generator().manual_seed(1)) + 0.5).to(DEV).requires_grad_(True)
    y = mdn.relu_dropout(x, p, True, seed=1234)
    kept = y != 0
    frac = kept.double().mean().item()
    assert abs(frac - 0.9) <= 5 * (0.9 * 0.1 / N) ** 0.5, frac
    xs, ys = x.detach()[kept].double(), y.detach()[kept].double()
    assert ((ys - xs / 0.9).abs() <= 1e-6 * xs / 0.9).all()
    # the mask is mtts.dropout's for the same seed
    same = D.apply_mask(x.detach(), p, 1234, seed_in=D.device_base(DEV))
    assert torch.equal(same, y.detach())
    # backward: zeros coincide with the forward's, survivors carry 1 / (1 - p)
    g = torch.rand(N, device=DEV) + 0.5
    y.backward(g)
    assert torch.equal(x.grad != 0, kept)
    assert ((x.grad[kept].double() - g[kept].double() / 0.9).abs() <= 1e-6 * g[kept].double() / 0.9).all()
    # negative inputs are dropped by the ReLU whatever the mask says; odd length (a tail past the 16-byte pieces)
    z = torch.randn(1001, generator=torch.Generator().manual_seed(2)).to(DEV)
    yz = mdn.relu_dropout(z, p, True, seed=99)
    assert (yz[z <= 0] == 0).all() and (yz >= 0).all()
    keep_z = D.apply_mask(torch.ones(1008, device=DEV), p, 99, seed_in=D.device_base(DEV))[:1001] != 0
    assert torch.equal(yz != 0, keep_z & (z > 0))
    # bf16 takes the same mask
    yb = mdn.relu_dropout(x.detach().to(BF16), p, True, seed=1234)
    assert torch.equal(yb != 0, kept)


# ---- sampler ----------------------------------------------------------------------------

def sampler_inputs(B, K, d, mode, seed):
    g = torch.Generator().manual_seed(seed)
    pi = torch.softmax(1.5 * torch.randn(B, K, generator=g), -1)
    mu = torch.randn(B, K, d, generator=g)
    sigma = 0.2 + torch.rand(R.sigma_shape(mode, B, K, d), generator=g)
    if mode == "fixed":
        sigma = torch.full((B,), 0.1)
    return pi, mu, sigma


SAMPLE_SEEDS = [17, -3, 2 ** 62 + 5, 123456789, 0]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", R.MODES)
def test_sampler_matches_the_restatement(mode, dtype):
    from mtts import mdn
    B, K, d = 5, 5, 41
    pi, mu, sigma = sampler_inputs(B, K, d, mode, 40)
    (pd, p64), (md, m64), (sd, s64) = (rounded(t, dtype) for t in (pi, mu, sigma))
    seeds = torch.tensor(SAMPLE_SEEDS, dtype=torch.int64, device=DEV)
    draws = torch.tensor([0, 1, 2, 7, 2 ** 33], dtype=torch.int64, device=DEV)
    want, ks, _, margin = R.sample(p64.float().numpy(), m64.numpy(), s64.numpy(), mode,
                                   [s & R.M64 for s in SAMPLE_SEEDS], draws.tolist())
    assert (margin > 2.0 ** -20).all(), margin          # no uniform near a CDF boundary: the pick is exact in fp32
    assert len(set(ks.tolist())) > 1
    got, comp = mdn.mixture_sample(pd, md, sd, mode, seed=seeds, draw=draws, return_component=True, use_base=False)
    assert got.shape == (B, d) and got.dtype == dtype and not got.requires_grad
    assert comp.tolist() == ks.tolist()
    std_max = float(s64.max())
    err = (got.double().cpu() - torch.from_numpy(want)).abs().max().item()
    scale = float(np.abs(want).max())
    bound = 2e-5 * std_max + (2.0 ** -22 + (BF16_ULP if dtype == BF16 else 0.0)) * scale
    print(f"sample: max|err|={err:.3e} bound={bound:.3e}")
    assert err <= bound
    # the same seeds: the same draw; another draw count: another one
    again = mdn.mixture_sample(pd, md, sd, mode, seed=seeds, draw=draws, use_base=False)
    assert torch.equal(again, got)
    other = mdn.mixture_sample(pd, md, sd, mode, seed=seeds, draw=draws + 1, use_base=False)
    assert not torch.equal(other, got)
    # a row alone, and at another row index, bit for bit
    for r in range(B):
        alone = mdn.mixture_sample(pd[r:r + 1], md[r:r + 1], sd[r:r + 1], mode, seed=seeds[r:r + 1],
                                   draw=draws[r:r + 1], use_base=False)
        assert torch.equal(alone[0], got[r]), r
    perm = torch.tensor([4, 2, 0, 3, 1], device=DEV)
    moved = mdn.mixture_sample(pd[perm], md[perm], sd[perm], mode, seed=seeds[perm], draw=draws[perm], use_base=False)
    assert torch.equal(moved, got[perm])


def test_sampler_noise_is_box_muller_of_the_same_uniforms():
    from mtts import mdn
    B, d = 3, 20001                                    # an odd width: the last pair is half used
    seeds = [5, 2 ** 63 + 11, 77]
    z = mdn.mixture_sample(torch.ones(B, 1, device=DEV), torch.zeros(B, 1, d, device=DEV), torch.ones(B, device=DEV),
                           "isotropic_across_clusters",
                           seed=torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64,
                                             device=DEV), use_base=False)
    want = np.stack([R.normals(R.stream_key(s), d) for s in seeds])
    err = np.abs(z.double().cpu().numpy() - want).max()
    print(f"noise: max|err|={err:.3e}")
    assert err <= 2e-5
    assert np.abs(want).max() > 3.5                    # the tails are exercised


def test_sampler_advances_with_the_device_base():
    from mtts import dropout as D, mdn
    pi, mu, sigma = (t.to(DEV) for t in sampler_inputs(4, 5, 64, "isotropic", 41))
    a = mdn.mixture_sample(pi, mu, sigma, "isotropic", seed=9)
    b = mdn.mixture_sample(pi, mu, sigma, "isotropic", seed=9)
    assert torch.equal(a, b)
    # an integer seed gives row r the seed s + r * ROW_SEED_STEP, plus the device base: the restatement's draw
    # wherever its uniform is clear of the CDF boundaries
    base = int(D.device_base(DEV).item())
    want, _, _, margin = R.sample(pi.cpu().numpy(), mu.cpu().numpy(), sigma.cpu().numpy(), "isotropic",
                                  [(s + base) & R.M64 for s in R.row_seeds(9, 4)])
    clear = margin > 2.0 ** -20
    # the noise bound times the largest std (1.2) plus fp32's rounding of outputs below 8
    assert (a.double().cpu() - torch.from_numpy(want)).abs()[clear].max().item() <= 2e-5 * 1.2 + 2.0 ** -22 * 8
    D.advance()
    c = mdn.mixture_sample(pi, mu, sigma, "isotropic", seed=9)
    assert not torch.equal(a, c)
    torch.manual_seed(3)
    d1 = mdn.mixture_sample(pi, mu, sigma, "isotropic")
    torch.manual_seed(3)
    d2 = mdn.mixture_sample(pi, mu, sigma, "isotropic")
    assert torch.equal(d1, d2)                          # torch.manual_seed reproduces the default seed


# ---- module level -----------------------------------------------------------------------

def golden_module(golden, mode, dropout=0.0):
    import smsd
    g = golden("smsd.npz")
    m = smsd.SMSD(bert_model=None, bert_dim=24, style_dim=40, num_mixtures=5, hidden_dim=32, dropout=dropout,
                  variance_mode=mode)
    sd = {k[len(mode) + 4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"{mode}/sd/")}
    m.mdn_head.load_state_dict({k: v.float() for k, v in sd.items()})
    return m.to(DEV), sd, g


@pytest.mark.parametrize("mode", R.MODES)
def test_module_eval_matches_the_reference(golden, mode):
    m, sd, g = golden_module(golden, mode)
    m.eval()
    x = torch.from_numpy(g[f"{mode}/x"]).float().to(DEV)
    with torch.no_grad():
        y, (pi, mu, sigma) = m(x, return_params=True, seed=4)
    assert y.shape == (3, 40) and pi.shape == (3, 5) and mu.shape == (3, 5, 40)
    assert tuple(sigma.shape) == R.sigma_shape(mode, 3, 5, 40)
    rpi, rmu, rsig = R.head(sd, torch.from_numpy(g[f"{mode}/x"]), mode, 5, 40)
    for got, ref, rec, name in ((pi, rpi, g[f"{mode}/pi"], "pi"), (mu, rmu, g[f"{mode}/mu"], "mu"),
                                (sigma, rsig, g[f"{mode}/sigma"], "sigma")):
        check(got, ref, name)
        check(got, rec, name + " (recorded)")
    hp, hm, hs = m.mdn_head(x)
    assert torch.equal(hp, pi) and torch.equal(hm, mu) and torch.equal(hs, sigma)
    # the sample is the sampler's on these parameters, detached
    assert not y.requires_grad
    assert torch.equal(y, m.sample(pi, mu, sigma, seed=4))


@pytest.mark.parametrize("mode", R.MODES)
def test_module_training_gradients(golden, mode):
    """Training forward + backward with a given epsilon and dropout 0, B = 3
    in every mode (the default one included: the corrected broadcast)."""
    m, sd, g = golden_module(golden, mode)
    m.train()
    x, y = (torch.from_numpy(g[f"{mode}/{n}"]) for n in ("x", "y"))
    eps = None if mode == "fixed" else torch.from_numpy(g[f"{mode}/noise_eps"])
    loss = m(x.float().to(DEV), y_true=y.float().to(DEV), epsilon=None if eps is None else eps.float().to(DEV))
    loss.backward()
    sd64 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = R.mixture_nll(y, *R.head(sd64, x, mode, 5, 40, epsilon=eps), mode)
    ref.backward()
    check(loss, ref, "loss")
    for k, p in m.mdn_head.named_parameters():
        assert p.grad is not None, k
        check(p.grad, sd64[k].grad, "d " + k)


def test_module_training_step_in_a_graph_draws_fresh_values(golden):
    from mtts import dropout as D
    m, _, g = golden_module(golden, "isotropic", dropout=0.1)
    m.train()
    x = torch.from_numpy(g["isotropic/x"]).float().to(DEV)
    y = torch.from_numpy(g["isotropic/y"]).float().to(DEV)
    static = {}

    def step():
        D.advance()
        for p in m.parameters():
            p.grad = None
        loss = m(x, y_true=y)
        loss.backward()
        with torch.no_grad():
            static["style"] = m(x)
        static["loss"] = loss.detach()
        static["g"] = m.mdn_head.noise_net.noise_scale.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(static["loss"]) and torch.isfinite(static["g"]).all()
        seen.append((static["style"].clone(), static["loss"].clone()))
    assert not torch.equal(seen[0][0], seen[1][0])      # a fresh style vector
    assert not torch.equal(seen[0][1], seen[1][1])      # fresh NoiseNet noise and dropout masks


def test_noise_net_stand_alone():
    """NoiseNet on its own keeps the reference's interface: x in eval, x +
    noise_scale * epsilon in training, epsilon given or drawn (N(0, 1) from the
    sampler's generator, reproduced by torch.manual_seed)."""
    import smsd
    net = smsd.NoiseNet().to(DEV)
    x = torch.randn(64, 100, generator=torch.Generator().manual_seed(1)).to(DEV)
    eps = torch.randn(64, 100, generator=torch.Generator().manual_seed(2)).to(DEV)
    net.eval()
    assert net(x) is x
    net.train()
    check(net(x, eps), x.double() + 0.1 * eps.double(), "x + noise_scale * epsilon", rtol=1e-6)
    torch.manual_seed(5)
    a = net(x)
    torch.manual_seed(5)
    b = net(x)
    assert torch.equal(a, b) and a.shape == x.shape
    z = ((a - x) / 0.1).double()
    n = z.numel()
    assert abs(z.mean().item()) <= 5 / n ** 0.5 + 1e-4 and abs(z.var().item() - 1) <= 5 * (2 / n) ** 0.5 + 1e-3


# ---- harness --------------------------------------------------------------------------

SMALL = dict(d_model=64, d_style=16, dec_layers=2, dec_heads=4, d_ff=128, text_layers=2, text_heads=2, text_d_k=32,
             text_d_inner=128, dur_filter=64, style_heads=4, max_len=256, dropout=0.0)


def _harness(with_smsd, with_keys):
    import smsd
    import train_harness as th
    torch.manual_seed(0)
    models = th.build_models(DEV, **SMALL)
    head = None
    if with_smsd:
        gen = torch.Generator().manual_seed(9)       # its own generator: the models' inits stay the same
        head = smsd.SMSD(bert_model=None, bert_dim=24, style_dim=16, num_mixtures=5, hidden_dim=32, dropout=0.0)
        with torch.no_grad():
            for p in head.parameters():
                p.add_(0.05 * torch.randn(p.shape, generator=gen))
        head = head.to(DEV)
    step = th.TrainStep(models, lr=1e-3, smsd=head)
    batch = th.synthetic_batch(2, DEV, T_text=12, T_codec=24, T_ref=16, d_style=16, seed=2)
    if with_keys:
        gen = torch.Generator().manual_seed(10)
        batch["style_cls"] = torch.randn(2, 24, generator=gen).to(DEV)
        batch["spk_emb"] = torch.randn(2, 16, generator=gen).to(DEV)
    torch.manual_seed(1)
    return step, batch, head


def test_train_step_with_smsd():
    step, batch, head = _harness(True, True)
    before = {k: v.detach().clone() for k, v in head.mdn_head.named_parameters()}
    out = step(batch)
    assert torch.isfinite(out["smsd"]) and out["smsd"].item() != 0.0
    assert torch.isfinite(out["loss_total"])
    want = out["codec"] + 0.1 * out["dur"] + 0.5 * out["smsd"]
    assert abs(out["loss_total"].item() - want.item()) <= 1e-5 * abs(want.item())
    for k, v in head.mdn_head.named_parameters():
        assert not torch.equal(v.detach(), before[k]), f"{k} did not move"


def test_train_step_without_smsd_is_unchanged():
    """smsd=None, and a module given but a batch without its inputs, run the
    step as it was: the same losses bit for bit on a fixed seed, loss_smsd 0."""
    plain, batch, _ = _harness(False, False)
    a = plain(batch)
    idle, batch2, head = _harness(True, False)
    b = idle(batch2)
    for k in ("loss_total", "codec", "dur", "smsd"):
        assert torch.equal(a[k], b[k]), k
    assert a["smsd"].item() == 0.0
    assert all(p.grad is None for p in head.parameters())
