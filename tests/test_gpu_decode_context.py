"""The model half of a decode context (mtts/context.py DecodeContext): which
step it routes to at every dtype, row count, key count and split-key setting,
that a session's two engines share one context, and that an engine drops
everything that lives as long as its context in one place.

The decoder is that of test_gpu_long_keys.py (2 layers, d_model 512, 8 heads:
head dim 64, 256 keys per chunk), over KEYS = 520 keys and over 40, which is
inside the single-pass range."""
import pytest
import torch

from test_gpu_generate import DEV, V
from test_gpu_long_keys import DM, DS, KEYS, _decoder

pytestmark = pytest.mark.gpu
SHORT = 40
BF16, FP32 = "bf16", "fp32"
# (compute dtype, rows, keys, split-key routing): (fused, packed weight images, xpk), read off the predicates the
# engine had before the context owned them: fused iff bf16 and <= 32 rows; the weights packed iff fused; xpk iff
# fused and (keys inside the single-pass range, or the split-key kernel on).  The packed images of the
# conditioning (khm, gamma_p) exist iff xpk, and fuse_q is off throughout.
TABLE = {
    (BF16, 4, SHORT, True): (True, True, True), (BF16, 4, SHORT, False): (True, True, True),
    (BF16, 4, KEYS, True): (True, True, True), (BF16, 4, KEYS, False): (True, True, False),
    (BF16, 32, SHORT, True): (True, True, True), (BF16, 32, SHORT, False): (True, True, True),
    (BF16, 32, KEYS, True): (True, True, True), (BF16, 32, KEYS, False): (True, True, False),
    (BF16, 33, SHORT, True): (False, False, False), (BF16, 33, SHORT, False): (False, False, False),
    (BF16, 33, KEYS, True): (False, False, False), (BF16, 33, KEYS, False): (False, False, False),
    (FP32, 4, SHORT, True): (False, False, False), (FP32, 4, SHORT, False): (False, False, False),
    (FP32, 4, KEYS, True): (False, False, False), (FP32, 4, KEYS, False): (False, False, False),
    (FP32, 32, SHORT, True): (False, False, False), (FP32, 32, SHORT, False): (False, False, False),
    (FP32, 32, KEYS, True): (False, False, False), (FP32, 32, KEYS, False): (False, False, False),
    (FP32, 33, SHORT, True): (False, False, False), (FP32, 33, SHORT, False): (False, False, False),
    (FP32, 33, KEYS, True): (False, False, False), (FP32, 33, KEYS, False): (False, False, False),
}
# one routing switch of DecodeEngine.OPTIONS off, at bf16, 4 rows, KEYS keys, split-key routing on
SWITCHED = {"packed": (True, False, False), "xpacked": (True, True, False)}
_models = {}


def _model(cd):
    if cd not in _models:
        _models[cd] = _decoder(torch.bfloat16 if cd == BF16 else None)
    return _models[cd]


def _routed(cd, rows, keys, split):
    """(fused, every weight image there / none there, xpk) of a context built over idle rows; asserts the rest."""
    from mtts.conditioning import Conditioning
    from mtts.context import DecodeContext
    m = _model(cd)
    with torch.no_grad():
        cond = Conditioning.idle(rows, keys, m._cd(), torch.device(DEV), None, split)
        ctx = DecodeContext.build(m, cond, rows, True)
    assert ctx.cond is cond and ctx.rows == rows and len(ctx.layers) == 2
    packed = [p.packed is not None for p in ctx.projections()]
    assert len(packed) == 2 * 7 + 1 and len(set(packed)) == 1
    assert all(p.operand is (p.packed if packed[0] else p.w) for p in ctx.projections())
    for c in cond.layers:
        assert (c.khm is not None) == (c.vhm is not None) == (c.gamma_p is not None) == (c.beta_p is not None) == ctx.xpk
    assert ctx.fuse_q is False
    return ctx.fused, packed[0], ctx.xpk


@pytest.mark.parametrize("cd, rows, keys, split", list(TABLE))
def test_routing_table(cd, rows, keys, split):
    assert _routed(cd, rows, keys, split) == TABLE[cd, rows, keys, split]


@pytest.mark.parametrize("switch", list(SWITCHED))
def test_routing_switches_are_read_at_the_latch(switch):
    from mtts.decode import DecodeEngine
    was = DecodeEngine.OPTIONS[switch]
    try:
        DecodeEngine.OPTIONS[switch] = False
        assert _routed(BF16, 4, KEYS, True) == SWITCHED[switch]
    finally:
        DecodeEngine.OPTIONS[switch] = was


def test_a_sessions_engines_share_one_context():
    ses = _model(BF16).open_session(4, KEYS)
    assert ses.pre.ctx is ses.eng.ctx
    assert ses.pre.ctx.fused is True and ses.pre.ctx.fused == ses.eng.ctx.fused
    assert ses.pre.ctx.xpk is True and ses.pre.ctx.xpk == ses.eng.ctx.xpk
    for (c1, s1), (c4, s4) in zip(ses.pre.states, ses.eng.states):
        assert c1 is not c4 and s1 is not s4 and c1.data_ptr() != c4.data_ptr() and s1.data_ptr() != s4.data_ptr()
        assert (c1.shape[0], s1.shape[0], c4.shape[0], s4.shape[0]) == (1, 1, 4, 4)


CONTEXT_LIFETIME = ("ctx", "ctx_key", "ctx_refs", "ctx_versions", "graph", "out_buf", "gen_graphs", "gen", "states",
                    "tok_buf", "pos_buf", "pos32", "prefill_logits")


def _empty(v):
    return v is None or (isinstance(v, dict) and not v)


def test_reset_drops_everything_that_lives_with_the_context():
    m = _model(BF16)
    g = torch.Generator(device=DEV).manual_seed(5)
    text = torch.randn(4, KEYS, DM, device=DEV, generator=g)
    z = torch.randn(4, DS, device=DEV, generator=g)
    tok = torch.randint(0, V, (4, 1), device=DEV, generator=g)
    prompt = torch.randint(0, V, (4, 3), device=DEV, generator=g)
    m.reset_decode_cache()
    try:
        with torch.no_grad():
            first, states = m.decode_step(tok, text, z, [None, None], 0)
            m.decode_step(tok, text, z, states, 1)
            m.generate(text, z, max_new_tokens=4, prompt_tokens=prompt)
            eng = m._engine
            for name in CONTEXT_LIFETIME:                   # the same conditioning: generate() kept the step's context
                assert not _empty(getattr(eng, name)), name
            eng.reset()
            for name in CONTEXT_LIFETIME:
                assert _empty(getattr(eng, name)), name
            again, _ = m.decode_step(tok, text, z, [None, None], 0)
        assert torch.equal(again, first)
    finally:
        m.reset_decode_cache()
