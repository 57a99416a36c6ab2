"""
Style Mixture Semantic Density (SMSD) module — MI355X-native drop-in for the
reference's smsd.py (same classes, constructor arguments and defaults, method
names, return shapes and state_dict keys).  ControlSpeech (arXiv:2406.01205)
section 3.3: a K-component Gaussian mixture over the style vector, predicted
from the BERT [CLS] embedding of a style description.

Everything trainable runs on libmtts: the MLP on ops.layer_norm (an any-width
row kernel of csrc/mdn.hip where bert_dim is not a multiple of 64) and
mtts.linear.linear, its ReLU -> Dropout pairs in one HIP pass each
(mtts_relu_dropout), softmax + NoiseNet + softplus in one (mtts_mdn_params_*),
the mixture NLL and its gradients (mtts_mixture_nll_*) and the sampler
(mtts_mixture_sample).  CPU tensors raise, as for every libmtts op.

Three documented departures from the reference:

1. The corrected broadcast.  In the default mode ("isotropic_across_clusters")
   the reference adds `-0.5 * d * log(variance)` of shape (B,) to a (B, K)
   tensor (:322-327): right for B == 1, row b's log-variance applied to
   COMPONENT b for B == K, an error for any other B.  Here row b's
   log-variance serves every component of row b, the formula its comment
   documents, at every B.  That equals the reference at B == 1 and in the
   other three modes at every B; it differs at B == K and runs where the
   reference raises.
2. The detached sample.  `SMSD.sample` returns a vector without gradient
   (the reference's is differentiable in mu and sigma; train.py calls it
   under no_grad).  Its draws are counter-based, not torch.multinomial /
   randn_like: reproducible per request from `seed` (an int, or one int64
   per row), the same in any row of any batch.
3. `bert_model=None` and tensor input.  BERT is the one part that needs the
   network; it is frozen by default, so its [CLS] vectors can be computed once,
   offline.  `SMSD(bert_model=None)` builds no encoder (the state dict then
   holds the `mdn_head.*` keys only) and `forward` takes a (B, bert_dim)
   tensor of precomputed [CLS] vectors in place of the strings.  With a model
   name, `transformers` is imported on construction and the encoder is built
   as in the reference; `import smsd` itself never imports it.

Seeds: the default seed is mtts.dropout.new_seed() (torch's CPU generator, so
torch.manual_seed reproduces a run) plus the per-device base that
mtts.dropout.advance() moves: a step captured in a hipGraph draws a fresh
style and fresh NoiseNet noise on every replay when it calls advance() first.
"""

import torch
import torch.nn as nn

from mtts import mdn, ops
from mtts.linear import cast_scope, linear


class SMSD(nn.Module):
    def __init__(
        self,
        bert_model="bert-base-uncased",
        bert_dim=768,
        style_dim=256,
        num_mixtures=5,
        hidden_dim=512,
        dropout=0.1,
        variance_mode="isotropic_across_clusters",
        freeze_bert=True,
    ):
        super().__init__()
        self.style_dim = style_dim
        self.num_mixtures = num_mixtures
        self.variance_mode = variance_mode

        # 1. BERT style semantic encoder (reference :40-45); None: precomputed [CLS] vectors
        self.tokenizer = None
        self.bert = None
        if bert_model is not None:
            from transformers import AutoModel, AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(bert_model)
            self.bert = AutoModel.from_pretrained(bert_model)
            if freeze_bert:
                for param in self.bert.parameters():
                    param.requires_grad = False

        # 2. Mixture density head
        self.mdn_head = MDNHead(
            input_dim=bert_dim,
            style_dim=style_dim,
            num_mixtures=num_mixtures,
            hidden_dim=hidden_dim,
            dropout=dropout,
            variance_mode=variance_mode,
        )

    def encode_style_text(self, texts):
        """texts: str or list of str -> (B, bert_dim) [CLS] embeddings (reference :57-88)."""
        if self.bert is None:
            raise TypeError("SMSD was built with bert_model=None: pass a (B, bert_dim) tensor of precomputed "
                            "[CLS] vectors instead of style strings")
        if isinstance(texts, str):
            texts = [texts]
        encoded = self.tokenizer(texts, padding=True, truncation=True, return_tensors="pt", max_length=128)
        encoded = {k: v.to(self.bert.device) for k, v in encoded.items()}
        with torch.set_grad_enabled(self.bert.training):
            outputs = self.bert(**encoded)
        return outputs.last_hidden_state[:, 0, :]

    def forward(self, style_texts, y_true=None, return_params=False, *, seed=None, epsilon=None):
        """style_texts: a (B, bert_dim) tensor of [CLS] vectors, or strings
        when an encoder was built.  With y_true (B, style_dim): the scalar
        mixture NLL.  Without: the sampled (B, style_dim) vector (no
        gradient), plus (pi, mu, sigma) with return_params.  `seed`: int or
        (B,) int64 tensor for the draws (the sampler's and, in training, the
        NoiseNet's); `epsilon`: the NoiseNet noise instead of a drawn one."""
        x = style_texts if isinstance(style_texts, torch.Tensor) else self.encode_style_text(style_texts)
        seeds = mdn.row_seeds(seed, x.shape[0], x.device) if x.is_cuda else None
        pi, mu, sigma = self.mdn_head(x, seed=seeds, epsilon=epsilon)
        if y_true is not None:
            return mixture_nll_loss(y_true, pi, mu, sigma, self.variance_mode)
        y_sampled = self.sample(pi, mu, sigma, seed=seeds)
        if return_params:
            return y_sampled, (pi, mu, sigma)
        return y_sampled

    def sample(self, pi, mu, sigma, *, seed=None, draw=None):
        """pi (B, K), mu (B, K, style_dim), sigma by variance_mode ->
        (B, style_dim), detached (module docstring, departure 2)."""
        return mdn.mixture_sample(pi, mu, sigma, self.variance_mode, seed=seed, draw=draw)


class MDNHead(nn.Module):
    """BERT embedding (B, input_dim) -> (pi (B, K), mu (B, K, style_dim), sigma)."""

    def __init__(
        self,
        input_dim,
        style_dim,
        num_mixtures,
        hidden_dim,
        dropout=0.1,
        variance_mode="isotropic_across_clusters",
    ):
        super().__init__()
        mdn.mode_code(variance_mode)
        self.num_mixtures = num_mixtures
        self.style_dim = style_dim
        self.variance_mode = variance_mode

        self.mlp = nn.Sequential(
            nn.LayerNorm(input_dim),
            nn.Linear(input_dim, hidden_dim),
            nn.ReLU(),
            nn.Dropout(dropout),
            nn.Linear(hidden_dim, hidden_dim),
            nn.ReLU(),
            nn.Dropout(dropout),
        )
        self.pi_head = nn.Linear(hidden_dim, num_mixtures)
        self.mu_head = nn.Linear(hidden_dim, num_mixtures * style_dim)
        if variance_mode == "isotropic_across_clusters":
            self.sigma_head = nn.Linear(hidden_dim, 1)
        elif variance_mode == "isotropic":
            self.sigma_head = nn.Linear(hidden_dim, num_mixtures)
        elif variance_mode == "diagonal":
            self.sigma_head = nn.Linear(hidden_dim, num_mixtures * style_dim)
        else:  # fixed
            self.sigma_head = None
        if self.sigma_head is not None:
            self.noise_net = NoiseNet()

    def forward(self, x, *, seed=None, epsilon=None):
        """MLP -> three heads -> the parameter kernel, as the reference
        (:234-264).  `seed` / `epsilon`: the NoiseNet's drawn / given noise
        (training only)."""
        if not x.is_cuda:
            raise RuntimeError("libmtts ops need CUDA (HIP) tensors; there is no CPU path")
        B = x.shape[0]
        m = self.mlp
        with cast_scope():   # compute-dtype weight copies valid for this call (mtts.linear)
            if x.shape[-1] % 64 == 0:
                h, _ = ops.layer_norm(x, m[0].weight, m[0].bias, m[0].eps)
            else:   # a width ln.hip does not take (768 is one it does): the head's any-width row kernel
                h = mdn.layer_norm_rows(x, m[0].weight, m[0].bias, m[0].eps)
            h = mdn.relu_dropout(linear(h, m[1].weight, m[1].bias), m[3].p, self.training)
            h = mdn.relu_dropout(linear(h, m[4].weight, m[4].bias), m[6].p, self.training)
            pi_logits = linear(h, self.pi_head.weight, self.pi_head.bias)
            mu = linear(h, self.mu_head.weight, self.mu_head.bias).view(B, self.num_mixtures, self.style_dim)
            sigma_raw = noise_scale = None
            if self.sigma_head is not None:
                sigma_raw = linear(h, self.sigma_head.weight, self.sigma_head.bias)
                noise_scale = self.noise_net.noise_scale
        pi, sigma = mdn.mdn_params(pi_logits, sigma_raw, noise_scale, self.variance_mode, self.style_dim,
                                   training=self.training, epsilon=epsilon, seed=seed)
        return pi, mu, sigma


class NoiseNet(nn.Module):
    """x + noise_scale * epsilon in training, x in eval (reference :267-292).
    Inside MDNHead the perturbation is part of the parameter kernel; this
    stand-alone form keeps the reference's interface, with epsilon drawn by
    the same counter-based generator when it is not given."""

    def __init__(self, noise_scale=0.1):
        super().__init__()
        self.noise_scale = nn.Parameter(torch.tensor(noise_scale))

    def forward(self, x, epsilon=None):
        if not self.training:
            return x
        if epsilon is None:
            z = torch.zeros(x.shape[0], 1, x[0].numel(), device=x.device, dtype=x.dtype)
            epsilon = mdn.mixture_sample(torch.ones(x.shape[0], 1, device=x.device, dtype=x.dtype), z,
                                         torch.ones(x.shape[0], device=x.device, dtype=x.dtype),
                                         "isotropic_across_clusters").view(x.shape)
        return x + self.noise_scale * epsilon


def mixture_nll_loss(y_true, pi, mu, sigma, variance_mode="isotropic_across_clusters"):
    """Negative log-likelihood of y_true (B, d) under the mixture (pi (B, K),
    mu (B, K, d), sigma by mode): a scalar, reference :295-372 with the
    corrected broadcast of the default mode (module docstring, departure 1)."""
    return mdn.mixture_nll(y_true, pi, mu, sigma, variance_mode)
