"""float64 numpy reference of the slot form of the per-row token sampler
(include/mtts.h, mtts_sample_tokens_slots; csrc/sample.hip), shared by
tests/test_sample_slots_cpu.py (the reference on its own) and the GPU tests
(the kernel and the decode session against it).

It is sample_rows_ref.sample_rows_ref called one row at a time with
col = draw[r], so the stream, the filters and the penalty arithmetic are not
restated here, plus the bookkeeping of one launch: a row finished at entry
gets pad_id and keeps its history, draw and length; any other row writes its
token to history[r, draw[r]] (when the buffer has that column), grows draw and
length by one and finishes on eos_id or at max_length; and, with `advance`,
pos[r] grows by one only for rows unfinished AFTER the draw.
"""
import numpy as np

import sample_rows_ref as RR


def sample_slots_ref(logits, *, temperature, top_k, top_p, seed, draw, penalty=None, window=0, history=None,
                     bias=None, pad_id=0, eos_id=None, finished=None, length=None, max_length=None, pos=None,
                     advance=True, emitted=None):
    """Returns (tokens (rows,) int64, per-row acceptance sets, after), `after`
    a dict of the expected history / draw / length / finished / pos /
    unfinished once the launch is done (None for what was not given).
    `emitted` (rows,): the tokens the kernel under test drew -- the
    bookkeeping then follows them instead of the reference's own tokens (an
    ambiguous draw may differ, and eos_id depends on the token)."""
    logits = np.asarray(logits)
    rows, V = logits.shape
    tokens = np.empty(rows, dtype=np.int64)
    accept = []
    for r in range(rows):
        one = slice(r, r + 1)
        b = None if bias is None else (np.asarray(bias)[one] if np.asarray(bias).ndim == 2 else bias)
        t, a = RR.sample_rows_ref(
            logits[one], temperature=temperature[one], top_k=top_k[one], top_p=top_p[one], seed=seed[one],
            draw=draw[one], penalty=None if penalty is None else penalty[one], window=window,
            history=None if history is None else np.asarray(history)[one], col=int(draw[r]), bias=b, pad_id=pad_id,
            finished=None if finished is None else finished[one])
        tokens[r] = t[0]
        accept.append(a[0])
    used = tokens if emitted is None else np.asarray(emitted, dtype=np.int64)
    hist = None if history is None else np.array(history, dtype=np.int64)
    drawn = [int(x) for x in draw]
    lens = None if length is None else [int(x) for x in length]
    fin = None if finished is None else [int(x) for x in finished]
    for r in range(rows):
        if fin is not None and fin[r]:
            continue
        col = drawn[r]
        if hist is not None and 0 <= col < hist.shape[1]:
            hist[r, col] = used[r]
        drawn[r] += 1
        if lens is not None:
            lens[r] += 1
            if fin is not None and max_length is not None and lens[r] >= int(max_length[r]):
                fin[r] = 1
        if fin is not None and eos_id is not None and eos_id >= 0 and int(used[r]) == eos_id:
            fin[r] = 1
    p = None
    if pos is not None:
        p = [int(x) + (1 if advance and (fin is None or not fin[r]) else 0) for r, x in enumerate(pos)]
    after = dict(history=hist, draw=drawn, length=lens, finished=fin, pos=p,
                 unfinished=None if fin is None else rows - sum(1 for f in fin if f))
    return tokens, accept, after
