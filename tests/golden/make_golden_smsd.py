"""Writes tests/golden/smsd.npz: float64 values recorded from the REFERENCE's
smsd.py (MDNHead, NoiseNet, mixture_nll_loss), which the tests compare the
project's float64 restatement (tests/smsd_ref.py) and, through it, the HIP
kernels against.

RUN ONLY WHERE THE REFERENCE IS CHECKED OUT (it imports /root/reference/smsd.py;
no test does).  `python tests/golden/make_golden_smsd.py` rewrites the file;
the output is deterministic (fixed seeds, CPU, float64).

Small widths keep the file small: input_dim 24, hidden 32, style_dim 40, K 5.
Per variance mode m the file holds
    m/sd/<key>            the head's state dict (every parameter perturbed, so
                          LayerNorm's affine and the biases matter)
    m/x (3, 24), m/y (3, 40)
    m/pi, m/mu, m/sigma   MDNHead.forward(x) in eval mode ("fixed": the reference
                          builds 0.1 * ones(B) in fp32; stored as float64)
    m/noise_in, m/noise_eps, m/noise_out
                          NoiseNet in training mode on the head's own
                          sigma_raw with a recorded epsilon (not for "fixed")
    m/loss, m/g_pi, m/g_mu, m/g_sigma, m/g_y
                          mixture_nll_loss on the first Bl rows of (y, pi, mu,
                          sigma) and its autograd gradients; Bl = 1 for the
                          default mode (the reference's broadcast is the
                          documented formula only there), 3 for the others
    m/keys, m/shapes      state-dict key names and shapes at the reference
                          widths (768, 256, 5, 512), as strings
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "smsd.npz")
MODES = ("isotropic_across_clusters", "isotropic", "diagonal", "fixed")
IN, HID, D, K, B = 24, 32, 40, 5, 3


def main():
    sys.path.insert(0, REF)
    import smsd as ref
    out = {}
    for mi, mode in enumerate(MODES):
        torch.manual_seed(100 + mi)
        head = ref.MDNHead(IN, D, K, HID, dropout=0.1, variance_mode=mode).double().eval()
        with torch.no_grad():
            for p in head.parameters():
                p.add_(0.1 * torch.randn_like(p))
        for k, v in head.state_dict().items():
            out[f"{mode}/sd/{k}"] = v.numpy().copy()
        x = torch.randn(B, IN, dtype=torch.float64)
        y = torch.randn(B, D, dtype=torch.float64)
        with torch.no_grad():
            pi, mu, sigma = head(x)
        out.update({f"{mode}/x": x.numpy(), f"{mode}/y": y.numpy(), f"{mode}/pi": pi.numpy(),
                    f"{mode}/mu": mu.numpy(), f"{mode}/sigma": sigma.double().numpy()})
        if mode != "fixed":
            with torch.no_grad():
                sraw = head.sigma_head(head.mlp(x))
                eps = torch.randn_like(sraw)
                head.noise_net.train()
                nout = head.noise_net(sraw, eps)
                head.noise_net.eval()
            out.update({f"{mode}/noise_in": sraw.numpy(), f"{mode}/noise_eps": eps.numpy(),
                        f"{mode}/noise_out": nout.numpy()})
        Bl = 1 if mode == "isotropic_across_clusters" else B
        leaves = [t[:Bl].detach().clone().requires_grad_(True) for t in (y, pi, mu, sigma)]
        loss = ref.mixture_nll_loss(*leaves, variance_mode=mode)
        loss.backward()
        out[f"{mode}/loss"] = loss.detach().numpy()
        for name, t in zip(("y", "pi", "mu", "sigma"), leaves):
            if t.grad is not None:
                out[f"{mode}/g_{name}"] = t.grad.numpy()
        full = ref.MDNHead(768, 256, 5, 512, variance_mode=mode).state_dict()
        out[f"{mode}/keys"] = np.array(list(full.keys()))
        out[f"{mode}/shapes"] = np.array([",".join(str(n) for n in v.shape) for v in full.values()])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
