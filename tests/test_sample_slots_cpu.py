"""The float64 reference of the slot form of the sampler
(tests/sample_slots_ref.py) on hand-made cases: rows at different draw counts
write different columns and are penalised over their own windows, a finished
row leaves its history alone, and a row that finishes in this launch does not
advance."""
import numpy as np

import sample_rows_ref as RR
import sample_slots_ref as SL

V = 12


def _greedy(first):
    logits = np.zeros((len(first), V), dtype=np.float32)
    for r, t in enumerate(first):
        logits[r, t] = 5.0
    n = len(first)
    return logits, dict(temperature=[0.0] * n, top_k=[0] * n, top_p=[1.0] * n, seed=[1] * n)


def test_rows_at_different_draw_counts_write_different_columns():
    logits, ctl = _greedy([7, 9, 3])
    hist = np.full((3, 6), -7, dtype=np.int64)
    tok, acc, after = SL.sample_slots_ref(logits, draw=[0, 4, 6], history=hist, **ctl)
    assert tok.tolist() == [7, 9, 3] and acc == [{7}, {9}, {3}]
    want = np.full((3, 6), -7, dtype=np.int64)
    want[0, 0], want[1, 4] = 7, 9                           # row 2's column 6 is outside the buffer: no write
    assert np.array_equal(after["history"], want) and after["draw"] == [1, 5, 7]
    assert (hist == -7).all()                               # the input is left unchanged


def test_penalty_window_is_the_rows_own_last_columns():
    # token 7 leads by 5.0 over token 2 at 4.0: a penalty of 2 on 7 (-> 2.5) hands the row to 2
    logits = np.zeros((3, V), dtype=np.float32)
    logits[:, 7], logits[:, 2] = 5.0, 4.0
    ctl = dict(temperature=[0.0] * 3, top_k=[0] * 3, top_p=[1.0] * 3, seed=[1] * 3, penalty=[2.0] * 3)
    hist = np.zeros((3, 8), dtype=np.int64)
    hist[:, 1] = 7                                          # column 1 holds 7 in every row
    # row 0: draw 2, window 2 covers columns 0..1: penalised.  row 1: draw 5, window covers 3..4: not.
    # row 2: draw 1: its window is column 0 alone: not (column 1 is not its past).
    tok, _, _ = SL.sample_slots_ref(logits, draw=[2, 5, 1], history=hist, window=2, **ctl)
    assert tok.tolist() == [2, 7, 7]
    # the same through the rows form, one row at a time at its own column
    for r, (dr, want) in enumerate(zip([2, 5, 1], [2, 7, 7])):
        one = {k: v[r:r + 1] for k, v in ctl.items()}
        t, _ = RR.sample_rows_ref(logits[r:r + 1], draw=[dr], history=hist[r:r + 1], col=dr, window=2, **one)
        assert t.tolist() == [want]


def test_finished_row_leaves_its_history_alone():
    logits, ctl = _greedy([7, 9])
    hist = np.array([[4, 5, 6, -7], [4, 5, 6, -7]], dtype=np.int64)
    tok, acc, after = SL.sample_slots_ref(logits, draw=[3, 3], history=hist, pad_id=2, finished=[1, 0],
                                          length=[3, 3], max_length=[3, 9], pos=[2, 2], **ctl)
    assert tok.tolist() == [2, 9] and acc[0] == {2}
    assert after["history"].tolist() == [[4, 5, 6, -7], [4, 5, 6, 9]]
    assert after["draw"] == [3, 4] and after["length"] == [3, 4] and after["finished"] == [1, 0]
    assert after["pos"] == [2, 3] and after["unfinished"] == 1


def test_row_that_finishes_in_this_launch_does_not_advance():
    eos = 4
    logits, ctl = _greedy([7, eos, 9, 5])
    tok, _, after = SL.sample_slots_ref(logits, draw=[0, 2, 1, 0], eos_id=eos, finished=[0, 0, 0, 0],
                                        length=[0, 2, 1, 0], max_length=[1, 9, 9, 2], pos=[0, 8, 3, 5], **ctl)
    assert tok.tolist() == [7, eos, 9, 5]
    assert after["finished"] == [1, 1, 0, 0]                # row 0 at its cap, row 1 on eos
    assert after["pos"] == [0, 8, 4, 6] and after["length"] == [1, 3, 2, 1] and after["unfinished"] == 2
    # without finished every row advances
    _, _, free = SL.sample_slots_ref(logits, draw=[0, 2, 1, 0], pos=[0, 8, 3, 5], **ctl)
    assert free["pos"] == [1, 9, 4, 6] and free["finished"] is None
    # the bookkeeping follows the tokens the kernel emitted when they are given
    _, _, alt = SL.sample_slots_ref(logits, draw=[0, 2, 1, 0], eos_id=eos, finished=[0, 0, 0, 0],
                                    length=[0, 2, 1, 0], pos=[0, 8, 3, 5], emitted=[eos, 7, 9, 5], **ctl)
    assert alt["finished"] == [1, 0, 0, 0] and alt["pos"] == [0, 9, 4, 6]
