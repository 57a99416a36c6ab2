"""A/B of the SMSD mixture-density head at train.py's widths (bert_dim 768,
hidden 512, style_dim 256, K = 5, B = 8): the drop-in smsd.py on libmtts
against the same arithmetic in eager fp32 torch on the same device.

Three things are timed in one process, interleaved round by round so that a
busy host hits all of them alike:
    train   the training forward + backward (loss = smsd(x, y_true=y))
    sample  the inference sample under no_grad (smsd(x) in eval mode)
    torch   both of the above on eager torch modules (nn.LayerNorm / Linear /
            ReLU / Dropout, softmax, randn_like noise, softplus, the NLL with
            the corrected broadcast, multinomial + randn_like for the sample)
Each round times `--iters` calls of each between two device events after a
synchronise; the report gives the median over `--rounds` rounds with the
fastest and slowest round (the spread), and the device launches of one call
counted from a torch.profiler trace (kernels and copies).  No time bound
hangs on these numbers: the work per step is tiny and both paths are
launch-bound.

    python tools/smsd_ab.py --out profiles/smsd_ab.txt
"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mamba-tts-project_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


class TorchHead(nn.Module):
    """The head in eager torch (default variance mode, corrected broadcast)."""

    def __init__(self, bert_dim, style_dim, K, hidden, dropout):
        super().__init__()
        self.K, self.d = K, style_dim
        self.mlp = nn.Sequential(nn.LayerNorm(bert_dim), nn.Linear(bert_dim, hidden), nn.ReLU(), nn.Dropout(dropout),
                                 nn.Linear(hidden, hidden), nn.ReLU(), nn.Dropout(dropout))
        self.pi_head, self.mu_head = nn.Linear(hidden, K), nn.Linear(hidden, K * style_dim)
        self.sigma_head = nn.Linear(hidden, 1)
        self.noise_scale = nn.Parameter(torch.tensor(0.1))

    def params(self, x):
        h = self.mlp(x)
        pi = F.softmax(self.pi_head(h), dim=-1)
        mu = self.mu_head(h).view(x.shape[0], self.K, self.d)
        raw = self.sigma_head(h)
        if self.training:
            raw = raw + self.noise_scale * torch.randn_like(raw)
        return pi, mu, F.softplus(raw).squeeze(-1)

    def loss(self, x, y):
        pi, mu, sigma = self.params(x)
        var = (sigma ** 2).unsqueeze(-1)
        logp = (-0.5 * self.d * math.log(2 * math.pi) - 0.5 * self.d * torch.log(var)
                - 0.5 * ((y.unsqueeze(1) - mu) ** 2).sum(-1) / var)
        return -torch.logsumexp(torch.log(pi + 1e-8) + logp, dim=1).mean()

    def sample(self, x):
        pi, mu, sigma = self.params(x)
        k = torch.multinomial(pi, 1).squeeze(-1)
        sel = mu[torch.arange(x.shape[0], device=x.device), k]
        return sel + torch.randn_like(sel) * sigma.unsqueeze(-1)


def launches(fn):
    """Device launches (kernels + copies) of one call, from a profiler trace."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smsd_ab: no GPU; a timing needs one")
    import smsd
    dev = "cuda"
    torch.manual_seed(0)
    B, bert_dim, hidden, d, K = a.batch, 768, 512, 256, 5
    ours = smsd.SMSD(bert_model=None, bert_dim=bert_dim, style_dim=d, num_mixtures=K, hidden_dim=hidden).to(dev)
    ref = TorchHead(bert_dim, d, K, hidden, 0.1).to(dev)
    x, y = torch.randn(B, bert_dim, device=dev), torch.randn(B, d, device=dev)

    def zero(m):
        for p in m.parameters():
            p.grad = None

    def ours_train():
        ours.train()
        zero(ours)
        ours(x, y_true=y).backward()

    def ours_sample():
        ours.eval()
        with torch.no_grad():
            ours(x)

    def torch_train():
        ref.train()
        zero(ref)
        ref.loss(x, y).backward()

    def torch_sample():
        ref.eval()
        with torch.no_grad():
            ref.sample(x)

    cases = [("train  libmtts", ours_train), ("train  torch", torch_train), ("sample libmtts", ours_sample),
             ("sample torch", torch_sample)]
    for _, fn in cases:
        for _ in range(a.warmup):
            fn()
    times = {n: [] for n, _ in cases}
    for _ in range(a.rounds):
        for n, fn in cases:
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[n].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    lines = [f"SMSD head A/B: B={B} bert_dim={bert_dim} hidden={hidden} style_dim={d} K={K} fp32, "
             f"{torch.cuda.get_device_name(0)}",
             f"microseconds per call (host-paced: launches included), median of {a.rounds} interleaved rounds of "
             f"{a.iters} calls [fastest .. slowest round]; device launches of one call"]
    for n, fn in cases:
        t = times[n]
        try:
            nl = str(launches(fn))
        except Exception as e:     # the count is a side figure: say so rather than lose the timings
            nl = f"not measured ({type(e).__name__})"
        lines.append(f"  {n:15s} {statistics.median(t):8.1f} us  [{min(t):8.1f} .. {max(t):8.1f}]  launches {nl}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
