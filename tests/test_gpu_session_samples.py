"""n samples of one request in a decode session (DecodeSession.admit_samples,
open_session(share_keys=True), generate_requests' samples=n): member j gives
the tokens and log-probabilities of admit(slot, ..., seed=row_seeds(seed, n)[j])
alone in a plain session -- exactly, whether the members share one copy of the
K/V (mtts_attention_decode_split_shared) or hold copies; the slot that holds a
group's K/V stays reserved until every member has been taken; nothing captures
again.

The decoder is that of tests/test_gpu_long_keys.py (head dim 64: 256 keys per
chunk) with max_keys = 256 + 8, just past one chunk, so that the key side is
on the split-key kernel."""
import pytest
import torch

from test_gpu_generate import DEV, V
from test_gpu_generate_rows import WINDOW
from test_gpu_long_keys import CK, DM, DS, _decoder

pytestmark = pytest.mark.gpu
KEYS = CK + 8
SLOTS = 4
CAP = 12
EOS = 5


@pytest.fixture(scope="module")
def model():
    return _decoder(torch.bfloat16)


def _req(keys, i, cap=CAP, prompt=0, **kw):
    g = torch.Generator().manual_seed(500 + 7 * i + keys)
    r = dict(text_hidden=torch.randn(keys, DM, generator=g).to(DEV), z_style=torch.randn(DS, generator=g).to(DEV),
             max_new_tokens=cap, temperature=0.9, top_k=8, repetition_penalty=1.3)
    if prompt:
        r["prompt_tokens"] = torch.randint(0, V, (prompt,), generator=g).to(DEV)
    r.update(kw)
    return r


def _alone(ses, req, seed):
    """The request by admit() alone in `ses` (slot 0), run to its end."""
    ses.admit(0, seed=seed, **req)
    while 0 not in ses.poll():
        ses.run(1)
    return ses.take(0, return_logprobs=True) if ses.logprobs else (ses.take(0), None)


def _members(seed, n):
    from mtts.ops import row_seeds
    return row_seeds(seed, n)


def _run_out(ses):
    while any(s == "live" for s in ses.state):
        ses.run(1)
        ses.poll()


def _identity(ses):
    return ses.kv_rows.tolist() == list(range(ses.slots))


@pytest.mark.parametrize("prompt", [0, 5])
def test_members_equal_admit_alone(model, prompt):
    req, other = _req(KEYS - 3, 1, prompt=prompt), _req(40, 2)
    plain = model.open_session(SLOTS, KEYS, repetition_window=WINDOW, logprobs=True)
    refs = [_alone(plain, req, s) for s in _members(7, 3)]
    other_ref = _alone(plain, other, 11)
    assert len({tuple(t.tolist()) for t, _ in refs}) > 1                       # the members do differ
    for share in (True, False):
        ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW, logprobs=True, share_keys=share)
        ses.admit(1, seed=11, **other)                       # an unrelated request with another key count
        ses.admit_samples([3, 0, 2], seed=7, **req)
        if share:
            assert ses.kv_rows.tolist() == [3, 1, 3, 3]
            assert ses.kv_lens.tolist() == [1, 40, 1, KEYS - 3]
            k = ses.cond.layers[0].k
            assert not k[0].any() and not k[2].any() and k[3].any()             # one copy of the keys
        else:
            assert ses.kv_rows is None and ses.kv_lens.tolist() == [KEYS - 3, 40, KEYS - 3, KEYS - 3]
        _run_out(ses)
        for j, slot in enumerate([3, 0, 2]):
            toks, lps = ses.take(slot, return_logprobs=True)
            assert torch.equal(toks, refs[j][0]) and torch.equal(lps, refs[j][1]), (share, j)
        toks, lps = ses.take(1, return_logprobs=True)
        assert torch.equal(toks, other_ref[0]) and torch.equal(lps, other_ref[1])
        assert ses.state == ["idle"] * SLOTS and ses.captures == 1
        assert not share or _identity(ses)


def test_the_slot_that_holds_the_keys_stays_reserved(model):
    bias = torch.zeros(V)
    bias[EOS] = 2.0                                          # members end early, at lengths of their own
    req = _req(KEYS, 3, cap=24, temperature=1.0, top_k=0, repetition_penalty=1.0, logit_bias=bias.to(DEV))
    other = _req(30, 4)
    plain = model.open_session(SLOTS, KEYS, repetition_window=WINDOW, eos_id=EOS)
    # the set-up of this test: a seed at which member 0, whose slot holds the keys, ends before another member
    for seed in range(7, 15):
        refs = [_alone(plain, req, s)[0] for s in _members(seed, 3)]
        lengths = [t.numel() for t in refs]
        if lengths[0] < max(lengths[1:]):
            break
    assert lengths[0] < max(lengths[1:]), lengths
    ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW, eos_id=EOS, share_keys=True)
    ses.admit_samples([3, 0, 2], seed=seed, **req)
    while 3 not in ses.poll():
        ses.run(1)
    assert "live" in ses.state
    assert torch.equal(ses.take(3), refs[0])                 # the holder first
    assert ses.state[3] == "lent" and ses.kv_rows.tolist() == [3, 1, 3, 3]
    assert ses.cond.layers[0].k[3].any()            # its rows are still there for the others
    with pytest.raises(RuntimeError, match="slot 3"):
        ses.admit(3, seed=1, **other)
    with pytest.raises(RuntimeError, match="slot 3"):
        ses.admit_samples([1, 3], seed=1, **other)
    assert ses.state[1] == "idle" and ses.kv_rows.tolist() == [3, 1, 3, 3]      # the refused group wrote nothing
    with pytest.raises(RuntimeError):
        ses.take(3)
    _run_out(ses)
    assert torch.equal(ses.take(0), refs[1])                 # unchanged by the early take
    assert ses.state[3] == "lent" and ses.kv_rows.tolist() == [0, 1, 3, 3]
    with pytest.raises(RuntimeError, match="slot 3"):
        ses.admit(3, seed=1, **other)
    assert torch.equal(ses.take(2), refs[2])
    assert ses.state == ["idle"] * SLOTS and _identity(ses)
    assert not ses.cond.layers[0].k[3].any() and ses.kv_lens.tolist() == [1] * SLOTS
    ses.admit(3, seed=1, **other)                            # and now it is a slot like any other
    _run_out(ses)
    assert torch.equal(ses.take(3), _alone(plain, other, 1)[0])
    assert ses.captures == 1


def test_checks_come_before_any_write(model):
    ses = model.open_session(SLOTS, KEYS, repetition_window=WINDOW, share_keys=True)
    req = _req(20, 5)
    ses.admit(2, seed=1, **req)
    before = ses.cond.layers[0].k.clone()
    with pytest.raises(RuntimeError, match="slot 2"):
        ses.admit_samples([0, 2], seed=1, **req)
    with pytest.raises(ValueError):
        ses.admit_samples([0, 1], seed=1, **dict(req, temperature=-1.0))
    with pytest.raises(ValueError, match="max_keys"):
        ses.admit_samples([0, 1], seed=1, **_req(KEYS + 1, 5))
    with pytest.raises(ValueError, match="distinct"):
        ses.admit_samples([0, 0], seed=1, **req)
    with pytest.raises(ValueError):
        ses.admit_samples([0, SLOTS], seed=1, **req)
    assert ses.state == ["idle", "idle", "live", "idle"] and _identity(ses)
    assert torch.equal(ses.cond.layers[0].k, before) and ses.kv_lens.tolist() == [1, 1, 20, 1]


def test_share_keys_needs_the_split_key_routing(model, monkeypatch):
    from mtts.decode import DecodeEngine
    with pytest.raises(ValueError, match="single-pass"):
        model.open_session(SLOTS, CK, share_keys=True)
    model.open_session(SLOTS, CK + 1, share_keys=True)
    monkeypatch.setitem(DecodeEngine.OPTIONS, "split_keys", False)
    with pytest.raises(ValueError, match="split_keys"):
        model.open_session(SLOTS, KEYS, share_keys=True)


def test_generate_requests_with_samples(model):
    from mtts.session import plan_slots
    reqs = [dict(_req(KEYS, 10, cap=9), seed=3),
            dict(_req(50, 11, cap=6, prompt=4), seed=4, samples=3),
            dict(_req(KEYS - 1, 12, cap=11), seed=5, samples=1),
            dict(_req(17, 13, cap=5), seed=6),
            dict(_req(200, 14, cap=7), seed=8, samples=3)]
    caps = [r["max_new_tokens"] for r in reqs]
    want = [r.get("samples") for r in reqs]
    pre = ["prompt_tokens" in r for r in reqs]
    plain = model.open_session(SLOTS, KEYS, repetition_window=WINDOW, logprobs=True)
    expect = []
    for r in reqs:
        base = {k: v for k, v in r.items() if k not in ("samples", "seed")}
        if r.get("samples") is None:
            expect.append(_alone(plain, base, r["seed"]))
        else:
            expect.append([_alone(plain, base, s) for s in _members(r["seed"], r["samples"])])
    where_plan, replays_plan = plan_slots(caps, SLOTS, 4, pre, want)
    for share in (True, False):
        out, where, replays, lps = model.generate_requests(reqs, slots=SLOTS, max_keys=KEYS, check_every=4,
                                                           repetition_window=WINDOW, return_logprobs=True,
                                                           share_keys=share)
        assert where == where_plan and replays == replays_plan
        assert where[1] == [1, 2, 3] and isinstance(where[2], list) and isinstance(where[0], int)
        for i, r in enumerate(reqs):
            if want[i] is None:
                assert torch.equal(out[i], expect[i][0]) and torch.equal(lps[i], expect[i][1]), (share, i)
            else:
                assert len(out[i]) == want[i] == len(lps[i])
                for j in range(want[i]):
                    assert torch.equal(out[i][j], expect[i][j][0]) and torch.equal(lps[i][j], expect[i][j][1]), \
                        (share, i, j)
    with pytest.raises(ValueError, match="samples"):
        model.generate_requests([dict(reqs[0], samples=SLOTS + 1)], slots=SLOTS, max_keys=KEYS)
