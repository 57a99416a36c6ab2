"""The slot form of the per-row sampler (ops.sample_tokens_slots,
csrc/sample.hip) against its float64 reference (tests/sample_slots_ref.py):
one wave / four waves and their boundary at V = 256, rows at different draw
counts (0, 1, above the window) in one launch, finished rows and rows that
reach their cap in the launch, pos / step given and absent -- tokens in the
reference's acceptance sets, every piece of bookkeeping exact -- with the rows
form run on the same inputs beside it, so a regression in the shared kernel
shows."""
import numpy as np
import pytest
import torch

import sample_rows_ref as RR
import sample_slots_ref as SL
from test_gpu_sample_rows import _dev, _settings

pytestmark = pytest.mark.gpu
DEV = "cuda"
HC = 270          # history columns: above the largest draw count used (256 + 5)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _i64(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("V", [10, 64, 256, 257, 1024])
def test_grid_against_reference(V):
    from mtts import ops
    rng = np.random.RandomState(100 + V)
    g = torch.Generator().manual_seed(100 + V)
    launch, ambiguous, total = 0, 0, 0
    for dtype in (torch.float32, torch.bfloat16):
        for rows in (1, 3, 32):
            for w in (0, 8, 256):
                logits = (3 * torch.randn(rows, V, generator=g)).to(dtype)
                # ids from a small range: duplicates inside every window are the rule
                hist = rng.randint(0, min(V, 24), size=(rows, HC)).astype(np.int64)
                draws = [(0, 1, w + 5, 3, max(w, 2))[(launch + r) % 5] for r in range(rows)]
                fin = [1 if (launch + r) % 4 == 1 else 0 for r in range(rows)]
                length = list(draws)
                caps = [draws[r] + 1 if r % 3 == 0 else 10 ** 6 for r in range(rows)]    # reached in this launch
                pos0 = [d + 3 for d in draws] if launch % 2 == 0 else None
                ctl = _settings(7 * launch, rows, V)
                ctl.update(seed=rng.randint(-2 ** 62, 2 ** 62, size=rows).tolist(), draw=draws)
                lg = logits.float().numpy()
                d = _dev(dict(ctl, max_length=caps))
                hist_d, fin_d, len_d = torch.from_numpy(hist).to(DEV), _i32(fin), _i64(length)
                unf_d = _i32([-1])
                pos_d = None if pos0 is None else _i32(pos0)
                step_d = _i32([41]) if launch % 3 else None
                tok = ops.sample_tokens_slots(logits.to(DEV), window=w, history=hist_d, pad_id=1, finished=fin_d,
                                              length=len_d, unfinished=unf_d, pos=pos_d, step=step_d, advance=True,
                                              **d)
                tok = tok.cpu().numpy()
                want, acc, after = SL.sample_slots_ref(lg, window=w, history=hist, pad_id=1, finished=fin,
                                                       length=length, max_length=caps, pos=pos0, emitted=tok, **ctl)
                where = f"{dtype} rows {rows} w {w} launch {launch}"
                for r in range(rows):
                    assert int(tok[r]) in acc[r], (f"{where} row {r} draw {draws[r]} fin {fin[r]} "
                                                   f"{ {k: v[r] for k, v in ctl.items()} }: {tok[r]} not in "
                                                   f"{sorted(acc[r])} (reference {want[r]})")
                assert np.array_equal(hist_d.cpu().numpy(), after["history"]), where
                assert d["draw"].cpu().tolist() == after["draw"], where
                assert len_d.cpu().tolist() == after["length"], where
                assert fin_d.cpu().tolist() == after["finished"], where
                assert int(unf_d) == after["unfinished"], where
                if pos0 is not None:
                    assert pos_d.cpu().tolist() == after["pos"], where
                if step_d is not None:
                    assert int(step_d) == 42, where
                # the rows form on the same inputs: the shared column col, as before
                col = w + 2
                d2 = _dev(ctl)
                hist2 = torch.from_numpy(hist).to(DEV)
                tok2 = ops.sample_tokens_rows(logits.to(DEV), window=w, history=hist2, step=col, pad_id=1,
                                              finished=_i32(fin), **d2).cpu().numpy()
                _, acc2 = RR.sample_rows_ref(lg, window=w, history=hist, col=col, pad_id=1, finished=fin, **ctl)
                for r in range(rows):
                    assert int(tok2[r]) in acc2[r], f"rows form, {where} row {r}: {tok2[r]} not in {sorted(acc2[r])}"
                assert hist2[:, col].cpu().tolist() == tok2.tolist(), where
                assert d2["draw"].cpu().tolist() == [x + (0 if f else 1) for x, f in zip(draws, fin)], where
                ambiguous += sum(len(a) > 1 for a in acc)
                total += rows
                launch += 1
    print(f"V {V}: {ambiguous} of {total} rows have an ambiguous acceptance set")
    assert ambiguous <= 0.01 * total, (ambiguous, total)


def test_bookkeeping_over_launches_and_a_one_row_view():
    from mtts import ops
    V, rows, eos, pad = 12, 5, 4, 2
    # greedy rows, the argmax set by the logits: row 0 finished already (its tokens must survive), row 1 cap 1,
    # row 2 emits eos, row 3 runs on, row 4 reaches its cap at the second draw
    first = [7, 9, eos, 5, 6]
    logits = torch.zeros(rows, V, device=DEV)
    for r, t in enumerate(first):
        logits[r, t] = 5.0
    d = _dev(dict(temperature=[0.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[1] * rows,
                  draw=[3, 0, 0, 2, 0], max_length=[3, 1, 9, 9, 2]))
    fin, length = _i32([1, 0, 0, 0, 0]), _i64([3, 0, 0, 2, 0])
    unf, pos = _i32([-1]), _i32([2, 0, 0, 2, 0])
    hist = torch.full((rows, 5), -7, dtype=torch.int64, device=DEV)
    hist[0, :3] = torch.tensor([8, 8, 8])
    kw = dict(history=hist, advance=True, eos_id=eos, pad_id=pad, finished=fin, length=length, unfinished=unf,
              pos=pos, **d)
    tok = ops.sample_tokens_slots(logits, **kw)
    assert tok.cpu().tolist() == [pad, 9, eos, 5, 6]
    assert fin.cpu().tolist() == [1, 1, 1, 0, 0] and length.cpu().tolist() == [3, 1, 1, 3, 1]
    assert d["draw"].cpu().tolist() == [3, 1, 1, 3, 1] and int(unf) == 2
    assert pos.cpu().tolist() == [2, 0, 0, 3, 1]            # rows 1 and 2 ended in this launch: no advance
    tok = ops.sample_tokens_slots(logits, **kw)
    assert tok.cpu().tolist() == [pad, pad, pad, 5, 6]
    assert fin.cpu().tolist() == [1, 1, 1, 0, 1] and pos.cpu().tolist() == [2, 0, 0, 4, 1] and int(unf) == 1
    for _ in range(3):                                      # idling: nothing of a finished row moves
        tok = ops.sample_tokens_slots(logits, **kw)
    assert tok.cpu().tolist() == [pad, pad, pad, 5, pad]
    assert pos.cpu().tolist() == [2, 0, 0, 7, 1] and d["draw"].cpu().tolist() == [3, 1, 1, 7, 2]
    assert hist.cpu().tolist() == [[8, 8, 8, -7, -7], [9, -7, -7, -7, -7], [eos, -7, -7, -7, -7],
                                   [-7, -7, 5, 5, 5], [6, 6, -7, -7, -7]]   # row 3's columns 5, 6: outside, dropped
    # a one-row view of the same buffers (a session's admission): pointers offset to the slot, rows = 1
    r = 4
    fin[r:r + 1].zero_()
    length[r:r + 1].zero_()
    d["draw"][r:r + 1].zero_()
    one = {k: v[r:r + 1] for k, v in d.items()}
    out = torch.zeros(rows, 1, dtype=torch.int64, device=DEV)
    for want_pos in (2, 2):                                 # cap 2: the second draw ends the row, pos stays
        ops.sample_tokens_slots(logits[r:r + 1], history=hist[r:r + 1], advance=True, eos_id=eos, pad_id=pad,
                                finished=fin[r:r + 1], length=length[r:r + 1], pos=pos[r:r + 1], out=out[r:r + 1],
                                **one)
        assert pos.cpu().tolist() == [2, 0, 0, 7, want_pos]
    assert out[:, 0].cpu().tolist() == [0, 0, 0, 0, 6] and fin.cpu().tolist() == [1, 1, 1, 0, 1]
    assert hist[3].cpu().tolist() == [-7, -7, 5, 5, 5] and d["draw"].cpu().tolist() == [3, 1, 1, 7, 2]
    # without finished every row advances
    pos2 = _i32([0] * rows)
    free = _dev(dict(temperature=[0.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[1] * rows,
                     draw=[0] * rows))
    ops.sample_tokens_slots(logits, advance=True, pos=pos2, **free)
    assert pos2.cpu().tolist() == [1] * rows


def test_checks_before_any_launch():
    from mtts import _lib, ops
    rows, V = 4, 16
    logits = torch.zeros(rows, V, device=DEV)
    good = _dev(dict(temperature=[1.0] * rows, top_k=[0] * rows, top_p=[1.0] * rows, seed=[0] * rows,
                     draw=[0] * rows))
    hist = torch.zeros(rows, 8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="window"):
        ops.sample_tokens_slots(logits, window=257, history=hist, **good)
    with pytest.raises(ValueError, match="window"):
        ops.sample_tokens_slots(logits, window=4, **good)
    with pytest.raises(ValueError, match="step"):
        ops.sample_tokens_slots(logits, step=3, **good)
    with pytest.raises(ValueError, match="draw"):
        ops.sample_tokens_slots(logits, **dict(good, draw=good["draw"].long()))
    with pytest.raises(TypeError):
        ops.sample_tokens_slots(logits, step0=1, **good)    # there is no step0
    assert good["draw"].cpu().tolist() == [0] * rows        # nothing ran
    # the entry point's own checks (a caller that bypasses the binding)
    a = _lib.SampleRowsArgs()
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("mtts_sample_tokens_slots", a)
    out, pos = torch.zeros(rows, dtype=torch.int64, device=DEV), torch.zeros(rows, dtype=torch.int32, device=DEV)
    a.rows, a.vocab, a.dtype, a.ld, a.logits, a.tokens, a.tok_stride = rows, V, _lib.F32, V, logits.data_ptr(), \
        out.data_ptr(), 1
    for name in ("temperature", "top_k", "top_p", "seed", "draw"):
        setattr(a, name, good[name].data_ptr())
    a.advance, a.pos, a.pos_rows = 1, pos.data_ptr(), rows - 1
    with pytest.raises(RuntimeError, match="pos_rows"):
        _lib.call("mtts_sample_tokens_slots", a)
    assert pos.cpu().tolist() == [0] * rows and good["draw"].cpu().tolist() == [0] * rows
