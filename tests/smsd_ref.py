"""float64 restatement of the SMSD mixture-density head (smsd.py; csrc/mdn.hip,
include/mtts.h "SMSD mixture-density head"), shared by tests/test_smsd_cpu.py
(which checks it against the recorded reference values in
tests/golden/smsd.npz and its generators against the distributions they must
draw from) and tests/test_gpu_smsd.py (which checks the kernels against it).

Arithmetic: torch float64, differentiable, so gradients come from autograd.
    h        = relu(W2 relu(W1 LN(x) + b1) + b2)            (dropout off)
    pi       = softmax(Wp h + bp)
    mu       = (Wm h + bm) viewed (B, K, d)
    sigma    = softplus(Ws h + bs [+ noise_scale * eps])    (x above 20: x)
    log N_k  = -d/2 log(2 pi) - 1/2 sum_j log var - 1/2 sum_j (y_j - mu_kj)^2 / var
    loss     = -mean_b logsumexp_k(log(pi_bk + 1e-8) + log N_bk)
The default mode ("isotropic_across_clusters") uses row b's variance for
every component of row b at every B (the documented formula); the other
three modes are the reference's at every B.

Random numbers: numpy uint64, wrapping.
    key     = mix64(seed + draw * golden)
    n(t, i) = mix64((key ^ t * TAG_MUL) + i * golden) >> 40
    u(t, i) = (n + 0.5) * 2^-24
    pick    : u(1, 0); first k with u * total < cdf_k, cdf the sequential fp32
              sums of the fp32 pi, total the last of them; else K - 1
    z       : z[2j] = r cos(t), z[2j+1] = r sin(t), r = sqrt(-2 ln u(2, j)),
              t = 2 pi u(3, j); the NoiseNet eps the same on streams 4, 5
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

MODES = ("isotropic_across_clusters", "isotropic", "diagonal", "fixed")
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
TAG_MUL = 0xD6E8FEB86659FD93
TAG_COMP, TAG_Z, TAG_EPS = 1, 2, 4
ROW_SEED_STEP = 0x2545F4914F6CDD1D
M64 = (1 << 64) - 1


def sigma_shape(mode, B, K, d):
    return {"isotropic_across_clusters": (B,), "isotropic": (B, K), "diagonal": (B, K, d), "fixed": (B,)}[mode]


def sigma_raw_width(mode, K, d):
    return {"isotropic_across_clusters": 1, "isotropic": K, "diagonal": K * d, "fixed": 0}[mode]


# ------------------------------------------------------------------ arithmetic

def mlp(sd, x):
    h = F.layer_norm(x, x.shape[-1:], sd["mlp.0.weight"], sd["mlp.0.bias"], 1e-5)
    h = torch.relu(F.linear(h, sd["mlp.1.weight"], sd["mlp.1.bias"]))
    return torch.relu(F.linear(h, sd["mlp.4.weight"], sd["mlp.4.bias"]))


def params(pi_logits, sigma_raw, mode, K, d, noise_scale=None, epsilon=None):
    """(pi, sigma) from the heads' raw outputs; epsilon given = training."""
    B = pi_logits.shape[0]
    pi = torch.softmax(pi_logits, dim=-1)
    if mode == "fixed":
        # the reference's placeholder is torch.ones(B) * 0.1, an fp32 tensor whatever the model's dtype
        return pi, torch.full((B,), 0.1, dtype=torch.float32).to(pi_logits.dtype)
    if epsilon is not None:
        sigma_raw = sigma_raw + noise_scale * epsilon.reshape(sigma_raw.shape)
    return pi, F.softplus(sigma_raw).reshape(sigma_shape(mode, B, K, d))


def head(sd, x, mode, K, d, epsilon=None):
    """MDNHead.forward on a float64 state dict: (pi, mu, sigma)."""
    h = mlp(sd, x)
    pi_logits = F.linear(h, sd["pi_head.weight"], sd["pi_head.bias"])
    mu = F.linear(h, sd["mu_head.weight"], sd["mu_head.bias"]).view(x.shape[0], K, d)
    sraw = None if mode == "fixed" else F.linear(h, sd["sigma_head.weight"], sd["sigma_head.bias"])
    pi, sigma = params(pi_logits, sraw, mode, K, d, sd.get("noise_net.noise_scale"), epsilon)
    return pi, mu, sigma


def mixture_nll(y, pi, mu, sigma, mode):
    B, K, d = mu.shape
    diff2 = (y.unsqueeze(1) - mu) ** 2
    if mode == "isotropic_across_clusters":
        var = (sigma ** 2).view(B, 1)
        logp = -0.5 * d * torch.log(var) - 0.5 * diff2.sum(-1) / var
    elif mode == "isotropic":
        var = sigma ** 2
        logp = -0.5 * d * torch.log(var) - 0.5 * diff2.sum(-1) / var
    elif mode == "diagonal":
        var = sigma ** 2
        logp = -0.5 * torch.log(var).sum(-1) - 0.5 * (diff2 / var).sum(-1)
    else:
        logp = -0.5 * d * math.log(0.01) - 0.5 * diff2.sum(-1) / 0.01
    logp = logp - 0.5 * d * math.log(2 * math.pi)
    return -torch.logsumexp(torch.log(pi + 1e-8) + logp, dim=1).mean()


def nll_and_grads(y, pi, mu, sigma, mode):
    """loss and d loss / d (y, pi, mu, sigma) (sigma's is None for "fixed")."""
    leaves = [t.detach().clone().double().requires_grad_(True) for t in (y, pi, mu, sigma)]
    loss = mixture_nll(*leaves, mode)
    loss.backward()
    g = [t.grad for t in leaves]
    return loss.detach(), g[0], g[1], g[2], (None if mode == "fixed" else g[3])


# --------------------------------------------------------------------- streams

def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def stream_key(seed, draw=0):
    return mix64(np.uint64(((int(seed) & M64) + (int(draw) & M64) * int(GOLDEN)) & M64))


def uniforms(key, tag, idx):
    """u(tag, i) float64 for the index array idx."""
    i = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64((np.uint64(key) ^ np.uint64((tag * TAG_MUL) & M64)) + i * GOLDEN)
    return ((h >> np.uint64(40)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(key, n, tag=TAG_Z):
    """z[0 .. n) float64 of one (seed, draw) stream."""
    j = np.arange((n + 1) // 2)
    r = np.sqrt(-2.0 * np.log(uniforms(key, tag, j)))
    t = 2.0 * np.pi * uniforms(key, tag + 1, j)
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1).reshape(-1)[:n]


def row_seeds(seed, rows):
    """The rows' seeds of one integer seed (mtts.mdn.row_seeds)."""
    return [((int(seed) & M64) + r * ROW_SEED_STEP) & M64 for r in range(rows)]


def pick(pi_row, key):
    """(k, margin): the component of one row and the distance of u * total to
    the nearest CDF boundary (the draw is exact in fp32 when that is well
    above fp32's rounding of the products)."""
    p = np.asarray(pi_row, dtype=np.float32)
    cdf = np.empty(len(p), dtype=np.float32)
    acc = np.float32(0)
    for k in range(len(p)):
        acc = np.float32(acc + p[k])
        cdf[k] = acc
    u = float(uniforms(key, TAG_COMP, [0])[0])
    t = u * float(cdf[-1])
    below = np.nonzero(t < cdf[:-1].astype(np.float64))[0]
    k = int(below[0]) if len(below) else len(p) - 1
    margin = float(np.min(np.abs(t - cdf[:-1].astype(np.float64)))) if len(p) > 1 else 1.0
    return k, margin


def sample(pi, mu, sigma, mode, seeds, draws=None):
    """(y (B, d), k (B,), z (B, d), margin (B,)) float64 numpy: the sampler on
    float64 copies of the given tensors."""
    pi, mu = np.asarray(pi, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    sigma = None if sigma is None else np.asarray(sigma, dtype=np.float64)
    B, K, d = mu.shape
    y, ks, zs, ms = np.empty((B, d)), np.empty(B, dtype=np.int64), np.empty((B, d)), np.empty(B)
    for b in range(B):
        key = stream_key(seeds[b], 0 if draws is None else draws[b])
        k, ms[b] = pick(pi[b], key)
        z = normals(key, d)
        std = {"isotropic_across_clusters": lambda: sigma[b], "isotropic": lambda: sigma[b, k],
               "diagonal": lambda: sigma[b, k], "fixed": lambda: 0.1}[mode]()
        y[b], ks[b], zs[b] = mu[b, k] + std * z, k, z
    return y, ks, zs, ms


def noise_eps(seeds, width):
    """(B, width) float64: the NoiseNet eps the parameter kernel draws."""
    return np.stack([normals(stream_key(s, 0), width, TAG_EPS) for s in seeds])
