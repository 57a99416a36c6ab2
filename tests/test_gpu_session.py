"""Continuous batching (mtts/session.py DecodeSession, generate_requests) on
the small decoder of tests/test_gpu_generate.py: the slot sampler inside the
session against its float64 reference, a request's tokens independent of its
company and of the schedule (exact), the session against generate() on the
request alone (exact), the queue against solo runs and the refill policy, the
admission checks, and generate() / decode_step left alone."""
import numpy as np
import pytest
import torch

import sample_slots_ref as SL
from test_gpu_generate import DEV, V, _model
from test_gpu_generate_rows import MIXED, PENALTY, WINDOW

pytestmark = pytest.mark.gpu
SLOTS, KEYS, D, DS = 3, 16, 64, 16
LENS = (12, 9, 5)
CAPS7 = [40, 6, 9, 7, 30, 5, 8]


def _request(i, cap, **over):
    """Request i: its own text (LENS[i % 3] keys), style, seed and controls (MIXED / PENALTY of the rows tests)."""
    g = torch.Generator().manual_seed(50 + i)
    r = dict(text_hidden=torch.randn(LENS[i % 3], D, generator=g).to(DEV), z_style=torch.randn(DS, generator=g).to(DEV),
             max_new_tokens=cap, temperature=MIXED["temperature"][i % 3], top_k=MIXED["top_k"][i % 3],
             top_p=MIXED["top_p"][i % 3], seed=1000 + 7 * i, repetition_penalty=PENALTY[i % 3])
    r.update(over)
    return r


def _sampled(cap=40, **over):
    """The request of the company tests: sampled, filtered, penalised."""
    return _request(1, cap, **over)


def _solo(ses, slot, req):
    ses.admit(slot, **req)
    pt = req.get("prompt_tokens")
    ses.run(req["max_new_tokens"] - (1 if pt is not None and pt.shape[-1] > 1 else 0))
    assert slot in ses.poll()
    return ses.take(slot)


@pytest.mark.parametrize("mode,cd", [("graph", torch.bfloat16), ("eager", torch.bfloat16), ("graph", None),
                                     ("eager", None)])
def test_slot_sampler_inside_the_session(mode, cd):
    m = _model(cd)
    m.decode_mode = mode
    ses = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    assert ses.eng.ctx.fused == (cd == torch.bfloat16)
    assert ses.captures == (1 if mode == "graph" else 0)
    reqs = [_request(0, 30), _request(1, 36), _request(2, 20)]
    ctl = dict(temperature=[r["temperature"] for r in reqs], top_k=[r["top_k"] for r in reqs],
               top_p=[r["top_p"] for r in reqs], seed=[r["seed"] for r in reqs],
               penalty=[r["repetition_penalty"] for r in reqs])
    caps = [r["max_new_tokens"] for r in reqs]
    ses.admit(0, **reqs[0])
    ses.admit(1, **reqs[1])
    live = [True] * SLOTS
    logits0 = ses.logits
    for t in range(40):
        if t == 5:
            ses.admit(2, **reqs[2])                         # five replays late: the rows sit at different columns
        draw, fin = ses.g["draw"].cpu().tolist(), ses.finished.cpu().tolist()
        hist, length = ses.g["hist"].cpu().numpy(), ses.length.cpu().tolist()
        pos = ses.eng.step_pos.cpu().tolist()
        ses.run(1)
        lg = ses.logits.float().cpu().numpy()
        tok = ses.eng.tok_buf[:, 0].cpu().numpy()
        _, acc, after = SL.sample_slots_ref(lg, draw=draw, window=WINDOW, history=hist, finished=fin, length=length,
                                            max_length=caps, pos=pos, emitted=tok, **ctl)
        for r in range(SLOTS):
            if fin[r] or not live[r]:
                continue
            assert int(tok[r]) in acc[r], f"slot {r} replay {t}: {tok[r]} not in {sorted(acc[r])}"
            if len(acc[r]) > 1:
                live[r] = False
        assert np.array_equal(ses.g["hist"].cpu().numpy(), after["history"]), t
        assert ses.g["draw"].cpu().tolist() == after["draw"] and ses.finished.cpu().tolist() == after["finished"], t
        assert ses.eng.step_pos.cpu().tolist() == after["pos"], t
    assert ses.logits is logits0                            # the logits buffer is static
    assert sum(live) >= SLOTS - 1, live
    assert sorted(ses.poll()) == [0, 1, 2]
    assert [int(ses.take(s).numel()) for s in range(SLOTS)] == caps
    assert ses.captures == (1 if mode == "graph" else 0)


def test_a_request_does_not_depend_on_its_company():
    m = _model()                                            # max_len 256
    req = _sampled()
    a = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    want = _solo(a, 1, req)                                 # slot 1 of an otherwise idle session
    assert want.shape == (40,) and want.dtype == torch.int64 and len(torch.unique(want)) > 3
    plain = _solo(a, 1, _sampled(repetition_penalty=None))
    assert not torch.equal(plain, want)                     # the penalty bites on this request
    b = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    b.admit(0, **_request(0, 100))
    b.admit(2, **_request(2, 80))
    b.run(17)                                               # the neighbours are 17 tokens in
    assert torch.equal(_solo(b, 1, req), want)
    other = _solo(b, 1, _request(3, 23, seed=5))            # another request through slot 1 ...
    assert other.shape == (23,)
    assert torch.equal(_solo(b, 1, req), want)              # ... and right after it was taken
    assert b.poll() == [0, 2] and b.captures == 1           # the neighbours ended meanwhile, at their caps
    assert b.take(0).shape == (100,) and b.take(2).shape == (80,)
    c = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    c.run(300)                                              # idle past pos_embed's 256 rows: positions must not move
    assert c.poll() == []                                   # (an IndexError here is the error flag)
    assert torch.equal(_solo(c, 1, req), want)
    assert c.eng.pos32.cpu().tolist() == [0, 0, 0]


def test_packed_step_slots_in_both_halves_of_the_image():
    """A d_model at which the packed step (_step_xpk) applies: the head-major
    K / V copies and the packed FiLM images are rewritten in place, for slots
    in the first and the second 16 rows of the packed image."""
    import mamba_decoder
    torch.manual_seed(0)
    dm = 512
    m = mamba_decoder.MambaTTSDecoder(V, d_model=dm, n_layers=2, n_heads=8, d_ff=512, d_style=DS,
                                      max_len=64).to(DEV).eval()
    m.compute_dtype = torch.bfloat16
    g = torch.Generator().manual_seed(9)

    def req(i, cap):
        return dict(text_hidden=torch.randn(LENS[i % 3], dm, generator=g).to(DEV),
                    z_style=torch.randn(DS, generator=g).to(DEV), max_new_tokens=cap, temperature=0.9, top_k=8,
                    seed=40 + i, repetition_penalty=1.3)

    r0, r1, r2 = req(0, 20), req(1, 30), req(2, 30)
    ses = m.open_session(20, KEYS, repetition_window=WINDOW)
    assert ses.eng.ctx.xpk and ses.cond.layers[0].khm is not None and ses.cond.layers[0].gamma_p is not None
    packed = ses.cond.layers[0].gamma_p.data
    want = _solo(ses, 1, r0)
    assert len(torch.unique(want)) > 3
    ses.admit(0, **r1)
    ses.admit(18, **r2)
    ses.run(7)
    assert torch.equal(_solo(ses, 17, r0), want)            # the second half of the image, with neighbours
    assert torch.equal(_solo(ses, 1, r0), want)
    assert ses.cond.layers[0].gamma_p.data is packed and ses.captures == 1
    text = torch.zeros(1, KEYS, dm, device=DEV)
    text[0, :LENS[0]] = r0["text_hidden"]
    mask = torch.zeros(1, KEYS, dtype=torch.bool, device=DEV)
    mask[0, :LENS[0]] = True
    toks, _ = m.generate(text, r0["z_style"][None], 20, text_mask=mask, temperature=[0.9], top_k=[8], seed=[40],
                         repetition_penalty=[1.3], repetition_window=WINDOW)
    assert torch.equal(toks[0], want)


def _padded(req):
    """The request as generate() takes it at batch 1: text and mask padded to KEYS."""
    S = req["text_hidden"].shape[0]
    text = torch.zeros(1, KEYS, D, device=DEV)
    text[0, :S] = req["text_hidden"]
    mask = torch.zeros(1, KEYS, dtype=torch.bool, device=DEV)
    mask[0, :S] = True
    return text, req["z_style"][None], mask


@pytest.mark.parametrize("cd", [torch.bfloat16, None])
@pytest.mark.parametrize("prompt", [False, True])
def test_session_equals_generate_on_the_request_alone(cd, prompt):
    m = _model(cd)
    ses = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    for i, cap in enumerate((24, 17, 31)):
        req = _request(i, cap)
        if prompt:
            req["prompt_tokens"] = torch.randint(0, V, (7,), generator=torch.Generator().manual_seed(3 + i)).to(DEV)
        got = _solo(ses, (i + 1) % SLOTS, req)
        text, z, mask = _padded(req)
        toks, lens = m.generate(text, z, cap, text_mask=mask, temperature=[req["temperature"]], top_k=[req["top_k"]],
                                top_p=[req["top_p"]], seed=[req["seed"]],
                                repetition_penalty=[req["repetition_penalty"]], repetition_window=WINDOW,
                                prompt_tokens=req["prompt_tokens"][None] if prompt else None)
        assert lens.tolist() == [cap] and got.shape == (cap,)
        assert torch.equal(got, toks[0]), (i, got.tolist(), toks[0].tolist())


def test_queue_follows_the_policy_and_equals_solo_runs():
    from mtts.session import DecodeSession, plan_slots
    m = _model()
    reqs = [_request(i, cap) for i, cap in enumerate(CAPS7)]
    before = DecodeSession.CAPTURES
    toks, where, replays = m.generate_requests(reqs, slots=SLOTS, max_keys=KEYS, check_every=4,
                                               repetition_window=WINDOW)
    assert DecodeSession.CAPTURES == before + 1             # exactly one graph was captured
    plan, count = plan_slots(CAPS7, SLOTS, 4)
    assert where == plan and replays == count and replays < 78
    assert [int(t.numel()) for t in toks] == CAPS7
    ses = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    for i, req in enumerate(reqs):
        assert torch.equal(_solo(ses, where[i], req), toks[i]), i
    assert len({tuple(t.tolist()[:5]) for t in toks}) > 3   # the requests differ
    # max_keys defaults to the longest conditioning; the schedule (check_every) influences no token
    toks2, where2, replays2 = m.generate_requests(reqs, slots=2, check_every=16, repetition_window=WINDOW)
    assert all(torch.equal(a, b) for a, b in zip(toks, toks2)) and replays2 == plan_slots(CAPS7, 2, 16)[1]


def test_eos_ends_a_request_before_its_cap():
    m = _model()
    eos, pad = 5, 2
    only = torch.full((V,), float("-inf"))
    only[eos] = 0.0                                         # this request can only emit eos
    never = torch.zeros(V)
    never[eos] = float("-inf")                              # these never do: they run to their caps
    reqs = [_request(0, 30, logit_bias=only), _request(1, 12, logit_bias=never), _request(2, 9, logit_bias=never),
            _request(3, 7, logit_bias=never)]
    ses = m.open_session(SLOTS, KEYS, eos_id=eos, pad_id=pad, repetition_window=WINDOW)
    ses.admit(0, **reqs[0])
    ses.admit(1, **reqs[1])
    ses.run(4)
    assert ses.poll() == [0] and ses.take(0).tolist() == [eos]
    assert ses.eng.tok_buf[:, 0].tolist()[0] == pad and ses.state == ["idle", "live", "idle"]
    ses.run(8)
    solo1 = ses.take(1)
    assert solo1.shape == (12,) and eos not in solo1.tolist()
    # the queue polls: the slot of the short request is refilled early, and no token changes
    toks, where, replays = m.generate_requests(reqs, slots=2, check_every=4, eos_id=eos, pad_id=pad,
                                               repetition_window=WINDOW)
    assert toks[0].tolist() == [eos] and [int(t.numel()) for t in toks[1:]] == [12, 9, 7]
    assert torch.equal(toks[1], solo1) and where[:3] == [0, 1, 0]
    for i in (2, 3):
        assert torch.equal(_solo(ses, 2, reqs[i]), toks[i]), i


def _snapshot(ses):
    out = [ses.kpm, ses.finished, ses.length, ses.eng.tok_buf, ses.eng.pos32, ses.eng.pos_buf]
    out += list(ses.g.values())
    for p in ses.cond.layers:
        out += [p.k, p.v, p.gamma, p.beta]
    for cs, ss in ses.eng.states:
        out += [cs, ss]
    return [t.clone() for t in out], out


def test_admission_checks_come_first():
    m = _model(max_len=64)
    ses = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    ses.admit(0, **_request(0, 20))
    ses.run(3)
    saved, bufs = _snapshot(ses)
    ok = _request(1, 10)
    long_text = torch.zeros(KEYS - 3, D, device=DEV)
    prompt = torch.zeros(10, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="max_keys"):
        ses.admit(1, **dict(ok, text_hidden=long_text, ref_hidden=torch.zeros(4, D, device=DEV)))
    with pytest.raises(ValueError, match="top_p"):
        ses.admit(1, **dict(ok, top_p=0.0))
    with pytest.raises(ValueError, match="repetition_penalty"):
        ses.admit(1, **dict(ok, repetition_penalty=float("inf")))
    with pytest.raises(ValueError, match="max_new_tokens"):
        ses.admit(1, **dict(ok, max_new_tokens=0))
    with pytest.raises(IndexError):
        ses.admit(1, **dict(ok, max_new_tokens=56, prompt_tokens=prompt))       # 10 + 56 - 1 > 64
    with pytest.raises(IndexError):
        ses.admit(1, **dict(ok, prompt_tokens=torch.tensor([3, V, 1], device=DEV)))
    with pytest.raises(IndexError):
        ses.admit(1, **dict(ok, start_token=V))
    with pytest.raises(RuntimeError, match="not been taken"):
        ses.admit(0, **ok)                                  # slot 0 is live
    with pytest.raises(RuntimeError):
        ses.take(1)                                         # nothing to take
    assert ses.captures == 1 and ses.state == ["live", "idle", "idle"]
    for was, now in zip(saved, bufs):
        assert torch.equal(was, now)                        # nothing was overwritten on the way to an error
    m.decode_mode = None
    with pytest.raises(RuntimeError):
        m.open_session(SLOTS, KEYS)
    m.decode_mode = "graph"
    ses.admit(1, **dict(ok, max_new_tokens=55, prompt_tokens=prompt))           # 10 + 55 - 1 == 64: the last position
    ses.run(54)
    assert sorted(ses.poll()) == [0, 1] and ses.take(1).shape == (55,) and ses.take(0).shape == (20,)
    ses.admit(2, **ok)
    ses.run(10)
    assert ses.poll() == [2]
    with pytest.raises(RuntimeError, match="not been taken"):
        ses.admit(2, **ok)                                  # finished and polled, but not taken


def test_generate_and_admit_refuse_the_same_requests():
    """Every bad request of test_admission_checks_come_first, plus positions
    past pos_embed, an out-of-range start token and a wrong-shaped logit_bias:
    generate() on the one-row batch and admit() raise the same exception type
    naming the same argument, and the session is left as it was.  (Too many
    keys is the one request generate() cannot refuse: max_keys is the
    session's own limit, so that row holds admit() to its message alone.)"""
    m = _model(max_len=64)
    ses = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    ses.admit(0, **_request(0, 20))
    ses.run(3)
    saved, bufs = _snapshot(ses)
    ok = _request(1, 10)
    prompt = torch.zeros(10, dtype=torch.long, device=DEV)
    bad = [  # (what changes in the request, exception, the argument both messages name)
        (dict(text_hidden=torch.zeros(KEYS - 3, D, device=DEV), ref_hidden=torch.zeros(4, D, device=DEV)), ValueError,
         None),                                             # too many keys: a session's limit, generate() has none
        (dict(top_p=0.0), ValueError, "top_p"),
        (dict(repetition_penalty=float("inf")), ValueError, "repetition_penalty"),
        (dict(max_new_tokens=0), ValueError, "max_new_tokens"),
        (dict(max_new_tokens=56, prompt_tokens=prompt), IndexError, "pos_embed"),       # 10 + 56 - 1 > 64
        (dict(start_token=V), IndexError, "start_token"),
        (dict(start_token=-1), IndexError, "start_token"),
        (dict(logit_bias=torch.zeros(V + 1, device=DEV)), ValueError, "logit_bias"),
        (dict(logit_bias=torch.zeros(2, V, device=DEV)), ValueError, "logit_bias"),
    ]
    for over, exc, arg in bad:
        req = dict(ok, **over)
        with pytest.raises(exc) as by_admit:
            ses.admit(1, **req)
        if arg is None:
            assert "max_keys" in str(by_admit.value)
            continue
        text, z, mask = _padded(req)
        one = {k: [req[k]] for k in ("temperature", "top_k", "top_p", "seed", "repetition_penalty")}
        pt = req.get("prompt_tokens")
        with pytest.raises(exc) as by_generate:
            m.generate(text, z, [req["max_new_tokens"]], text_mask=mask, repetition_window=WINDOW,
                       prompt_tokens=None if pt is None else pt[None], start_token=req.get("start_token", 0),
                       logit_bias=req.get("logit_bias"), **one)
        assert type(by_admit.value) is type(by_generate.value) is exc
        assert arg in str(by_admit.value) and arg in str(by_generate.value), (by_admit.value, by_generate.value)
    assert ses.captures == 1 and ses.state == ["live", "idle", "idle"]
    for was, now in zip(saved, bufs):
        assert torch.equal(was, now)                        # nothing was overwritten on the way to an error
    assert m._engine is None or not m._engine.gen_graphs    # and generate() captured nothing


def test_session_does_not_disturb_generate_or_decode_step():
    from test_gpu_generate import B, _conds
    m, fresh = _model(), _model()
    text, z, mask = _conds()
    seq = torch.randint(0, V, (B, 6), generator=torch.Generator().manual_seed(4)).to(DEV)

    def steps(model):
        out = []
        with torch.no_grad():
            states = [None] * 2
            for t in range(6):
                lg, states = model.decode_step(seq[:, t:t + 1], text, z, states, t, text_mask=mask)
                out.append(lg.clone())
        return torch.cat(out, 1)

    def gen(model):
        return model.generate(text, z, 20, text_mask=mask, repetition_penalty=PENALTY, repetition_window=WINDOW,
                              **MIXED)[0]

    lg_before, tok_before = steps(m), gen(m)
    engine = m._engine
    ses = m.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    req = _sampled()
    ses.admit(1, **req)
    ses.run(11)
    lg_during, tok_during = steps(m), gen(m)                # while the session is half way through a request
    ses.run(29)
    got = ses.take(1)
    assert m._engine is engine and len(engine.gen_graphs) == 1
    lg_after, tok_after = steps(m), gen(m)
    for lg, tok in ((lg_during, tok_during), (lg_after, tok_after)):
        assert torch.equal(lg, lg_before) and torch.equal(tok, tok_before)
    assert torch.equal(lg_after, steps(fresh)) and torch.equal(tok_after, gen(fresh))
    other = fresh.open_session(SLOTS, KEYS, repetition_window=WINDOW)
    assert torch.equal(_solo(other, 1, req), got)           # nor did they disturb the session
