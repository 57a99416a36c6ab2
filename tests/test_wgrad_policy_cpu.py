"""The deferred weight-gradient engine's flush policy (mtts/wgrad.py
makespan / utilisation / RoundQueue), without a device: C2's queue on 256
CUs, a 12-layer C2 backward simulated submit by submit, and the degenerate
queues."""
import pytest

from mtts import wgrad

CUS = 256
LONG, SHORT = 16384 // 64, 1024 // 64      # K-tiles: B*T tokens / the text K/V's B*T_text
# one C2 decoder layer in the order its backward submits: (output tiles, K-tiles, bytes of dy + x)
MB = 1 << 20
C2_LAYER = [
    [(32, LONG, 96 * MB)],                          # FFN down 1024 x 2048
    [(32, LONG, 96 * MB)],                          # FFN up 2048 x 1024
    [(16, LONG, 64 * MB)],                          # MHA out 1024 x 1024
    [(16, LONG, 64 * MB), (32, SHORT, 6 * MB)],     # q rows + text K/V rows of in_proj_weight: one submit
    [(32, LONG, 96 * MB)],                          # out_proj 1024 x 2048
    [(8, LONG, 66 * MB)],                           # dt_proj 2048 x 64
    [(8, LONG, 67 * MB)],                           # x_proj 96 x 2048
    [(64, LONG, 160 * MB)],                         # in_proj 4096 x 1024
]


def layers(n):
    return [(t, k) for _ in range(n) for sub in C2_LAYER for t, k, _ in sub]


def test_c2_layer_counts():
    one = layers(1)
    assert sum(t for t, k in one if k == LONG) == 208 and sum(t for t, k in one if k == SHORT) == 32
    assert sum(t * k for t, k in one) == 53760


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_one_to_five_c2_layers_leave_cus_idle(n):
    assert wgrad.utilisation(layers(n), CUS) == pytest.approx(0.8203125)
    assert wgrad.utilisation(layers(n), CUS) < wgrad.FILL


def test_six_c2_layers_fill_five_rounds():
    six = layers(6)
    assert wgrad.makespan(six, CUS) == 5 * LONG        # the 192 short tiles fit the last round's 32 free CUs
    u = wgrad.utilisation(six, CUS)
    assert u >= 0.98 and u == pytest.approx(6 * 53760 / (CUS * 5 * LONG))
    assert u >= wgrad.FILL


def test_twelve_layer_c2_backward_flushes_twice_in_ten_rounds():
    q = wgrad.RoundQueue()
    flushes = []
    n_submits = 0
    for _ in range(12):
        for sub in C2_LAYER:
            for t, k, nbytes in sub:
                q.add(t, k, nbytes)
            n_submits += 1
            if q.full(CUS):
                flushes.append((n_submits, list(q.work), q.held))
                q.clear()
    assert not q.work                                   # nothing left for the end-of-backward flush
    per_layer = len(C2_LAYER)
    assert [s for s, _, _ in flushes] == [6 * per_layer, 12 * per_layer]
    for _, work, held in flushes:
        assert len(work) == 54 <= wgrad.MAX_PROBLEMS and work == layers(6)
        assert held < wgrad.HOLD_BYTES                   # six layers' operands fit the byte cap
    rounds = sum(wgrad.makespan(w, CUS) for _, w, _ in flushes) / LONG
    assert rounds == 10


def _layers_until_flush(q, n_layers):
    for layer in range(n_layers):
        for sub in C2_LAYER:
            for t, k, nbytes in sub:
                q.add(t, k, nbytes)
            if q.full(CUS):
                return layer + 1
    return None


def test_plan_holds_only_what_fills_rounds_within_the_limits(monkeypatch):
    one = [(t, k) for sub in C2_LAYER for t, k, _ in sub]
    assert wgrad.plan_groups(one, 715 * MB, CUS) == 6
    assert _layers_until_flush(wgrad.RoundQueue(), 12) == 6
    # a byte cap below six layers: no number of layers fills rounds -> layer by layer, as before
    monkeypatch.setattr(wgrad, "HOLD_BYTES", 5 * 715 * MB)
    assert wgrad.plan_groups(one, 715 * MB, CUS) == 1
    assert _layers_until_flush(wgrad.RoundQueue(), 12) == 1
    monkeypatch.undo()
    # C5's decoder layer (d_model 512, 40960 tokens; text+reference K/V 41984): 80 tiles, 9 jobs
    k5, kv5 = 40960 // 64, 41984 // 64
    c5 = [(16, k5), (16, k5), (4, k5), (4, k5), (8, kv5), (8, k5), (4, k5), (4, k5), (16, k5)]
    assert sum(t for t, _ in c5) == 80
    for n in range(1, 7):
        assert wgrad.utilisation(c5 * n, CUS) < wgrad.FILL
    assert wgrad.plan_groups(c5 * 2, 2 * 1230 * MB, CUS) == 1


def test_problem_limit_flushes_whatever_the_plan():
    q = wgrad.RoundQueue()
    q.plan = 10 ** 6
    q.groups = 1
    for i in range(wgrad.MAX_PROBLEMS):
        q.add(1, LONG, 0)
        if q.full(CUS):
            break
    assert len(q.work) == wgrad.MAX_PROBLEMS - 2


def test_short_only_and_empty_queues():
    assert wgrad.utilisation([], CUS) == 0.0
    assert wgrad.makespan([], CUS) == 0
    assert wgrad.utilisation([(0, LONG)], CUS) == 0.0
    # 192 short tiles on 256 CUs: one short round, three quarters of the CUs busy
    assert wgrad.makespan([(192, SHORT)], CUS) == SHORT
    assert wgrad.utilisation([(192, SHORT)], CUS) == pytest.approx(0.75)
    # 300 short tiles: two short rounds
    assert wgrad.makespan([(300, SHORT)], CUS) == 2 * SHORT
    assert wgrad.utilisation([(300, SHORT)], CUS) == pytest.approx(300 / 512)


def test_makespan_matches_tile_by_tile_greedy():
    """The closed form for equal-K runs against the plain longest-first greedy."""
    import heapq
    import random
    rng = random.Random(3)
    for _ in range(50):
        cus = rng.choice([4, 16, 33, 256])
        work = [(rng.randint(0, 3 * cus), rng.choice([1, 2, 16, 40, 256])) for _ in range(rng.randint(1, 8))]
        loads = [0] * cus
        for k in sorted((k for t, k in work for _ in range(t)), reverse=True):
            heapq.heapreplace(loads, loads[0] + k)
        assert wgrad.makespan(work, cus) == max(loads), (cus, work)
