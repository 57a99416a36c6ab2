"""The refill policy of continuous batching (mtts.session.plan_slots), a pure
host function: every request scheduled once, no slot shared by two live
requests, and fewer replays than static batching needs."""
CAPS = [40, 6, 9, 7, 30, 5, 8]
SLOTS, CHECK = 3, 4


def _static_count(caps, slots):
    return sum(max(caps[i:i + slots]) for i in range(0, len(caps), slots))


def _intervals(caps, slots, check_every, where):
    """Replay the policy from its answer: (slot, admitted at replay, taken at
    replay) of every request, and the replay count."""
    free, live, out, nxt, t = set(range(slots)), {}, [None] * len(caps), 0, 0
    while nxt < len(caps) or live:
        while free and nxt < len(caps):
            s = where[nxt]
            assert s == min(free), (nxt, s, sorted(free))      # the lowest free slot, in request order
            free.remove(s)
            live[s] = [nxt, caps[nxt], t]
            nxt += 1
        n = min(check_every, max(v[1] for v in live.values()))
        t += n
        for s in sorted(live):
            live[s][1] -= n
            if live[s][1] <= 0:
                i, _, t0 = live.pop(s)
                out[i] = (s, t0, t)
                free.add(s)
    return out, t


def test_plan_on_the_issue_caps():
    from mtts.session import plan_slots
    where, replays = plan_slots(CAPS, SLOTS, CHECK)
    assert len(where) == len(CAPS) and all(0 <= s < SLOTS for s in where)       # every request exactly once
    spans, count = _intervals(CAPS, SLOTS, CHECK, where)
    assert count == replays
    for i, (s, t0, t1) in enumerate(spans):
        assert t1 - t0 >= CAPS[i]                                               # it got its replays
        for j, (s2, u0, u1) in enumerate(spans):
            if i < j and s == s2:
                assert t1 <= u0 or u1 <= t0, (i, j)                             # no slot holds two live requests
    static = _static_count(CAPS, SLOTS)
    assert static == 78
    assert replays < static, (replays, static)
    assert replays >= max(max(CAPS), -(-sum(CAPS) // SLOTS))                    # no schedule can do better


def test_plan_edges():
    import pytest
    from mtts.session import plan_slots
    assert plan_slots([5], 3, 16) == ([0], 5)
    assert plan_slots([3, 3, 3], 3, 2) == ([0, 1, 2], 3)                        # 2, then the 1 that is left
    assert plan_slots([4, 4], 1, 16) == ([0, 0], 8)
    assert plan_slots([], 2, 4) == ([], 0)
    # a prompt of more than one token draws its first token at admission
    assert plan_slots([4, 1], 1, 16, prefilled=[True, True]) == ([0, 0], 3)
    for bad in (dict(caps=[0], slots=1, check_every=1), dict(caps=[1], slots=0, check_every=1),
                dict(caps=[1], slots=1, check_every=0)):
        with pytest.raises(ValueError):
            plan_slots(**bad)
