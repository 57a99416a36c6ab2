"""The argument checks of the three sampler entry points (csrc/sample.hip),
without a GPU: every check runs before the first HIP call, so a struct that
fails one returns MTTS_EINVAL and leaves its message in mtts_last_error()
without touching a device.  One table of (entry point, the invalid fields,
the exact message); the two-fault rows pin which of two faults is reported,
i.e. the order in which the checks fire.

Every row MUST fail a check: a struct that passed them all would launch a
kernel on the host addresses below.  run() refuses a row that changes nothing,
and the base structs are never called as they are."""
import ctypes as C

import pytest

EINVAL = -22
ROWS, VOCAB = 4, 16
_BUF = (C.c_int64 * 64)()          # a host buffer whose address stands for every pointer; never dereferenced
PTR = C.addressof(_BUF)

SCALAR, PER_ROW, SLOTS = "sample_tokens", "sample_tokens_rows", "sample_tokens_slots"
ARRAYS = ("temperature", "top_k", "top_p", "seed", "draw")


def _base(entry):
    from mtts import _lib
    io = dict(rows=ROWS, vocab=VOCAB, dtype=_lib.F32, ld=VOCAB, logits=PTR, tokens=PTR, tok_stride=1, step=PTR,
              eos_id=-1, pad_id=0)
    if entry == SCALAR:
        return _lib.SampleArgs(temperature=1.0, top_k=0, top_p=1.0, seed=PTR, **io)
    return _lib.SampleRowsArgs(window=0, **{k: PTR for k in ARRAYS}, **io)


def _table():
    t = []
    for n in (SCALAR, PER_ROW, SLOTS):
        t += [
            (n, None, f"{n}: null pointer"),
            (n, dict(logits=None), f"{n}: null pointer"),
            (n, dict(tokens=None), f"{n}: null pointer"),
            (n, dict(dtype=2), f"{n}: dtype must be f32 or bf16"),
            (n, dict(dtype=-1), f"{n}: dtype must be f32 or bf16"),
            (n, dict(rows=0), f"{n}: rows=0 vocab={VOCAB} out of range"),
            (n, dict(vocab=0), f"{n}: rows={ROWS} vocab=0 out of range"),
            (n, dict(vocab=(1 << 24) + 1, ld=1 << 25), f"{n}: rows={ROWS} vocab={(1 << 24) + 1} out of range"),
            (n, dict(ld=VOCAB - 1), f"{n}: row stride below vocab"),
            (n, dict(bias=PTR, bias_ld=VOCAB - 1), f"{n}: row stride below vocab"),
            (n, dict(bias=PTR, bias_ld=-1), f"{n}: row stride below vocab"),
            (n, dict(pad_id=VOCAB), f"{n}: pad_id={VOCAB} / eos_id=-1 outside the vocabulary"),
            (n, dict(pad_id=-1), f"{n}: pad_id=-1 / eos_id=-1 outside the vocabulary"),
            (n, dict(eos_id=VOCAB), f"{n}: pad_id=0 / eos_id={VOCAB} outside the vocabulary"),
            (n, dict(history=PTR, hist_cols=8, hist_ld=4), f"{n}: bad history shape"),
            (n, dict(history=PTR, hist_cols=-1, hist_ld=4), f"{n}: bad history shape"),
            (n, dict(unfinished=PTR), f"{n}: unfinished needs finished"),
            # two faults: the earlier check is the one reported
            (n, dict(dtype=2, rows=0), f"{n}: dtype must be f32 or bf16"),
            (n, dict(vocab=0, ld=-1), f"{n}: rows={ROWS} vocab=0 out of range"),
            (n, dict(pad_id=VOCAB, history=PTR, hist_cols=8, hist_ld=4),
             f"{n}: pad_id={VOCAB} / eos_id=-1 outside the vocabulary"),
            (n, dict(history=PTR, hist_cols=8, hist_ld=4, unfinished=PTR), f"{n}: bad history shape"),
        ]
    n = SCALAR
    t += [
        (n, dict(temperature=-1.0), f"{n}: temperature=-1.000000 must be >= 0"),
        (n, dict(top_k=-1), f"{n}: top_k=-1 must be >= 0"),
        (n, dict(top_p=0.0), f"{n}: top_p=0.000000 must be in (0, 1]"),
        (n, dict(top_p=1.5), f"{n}: top_p=1.500000 must be in (0, 1]"),
        (n, dict(ld=VOCAB - 1, temperature=-1.0), f"{n}: row stride below vocab"),
        (n, dict(temperature=-1.0, top_k=-1), f"{n}: temperature=-1.000000 must be >= 0"),
        (n, dict(top_k=-1, top_p=1.5), f"{n}: top_k=-1 must be >= 0"),
        (n, dict(top_p=1.5, pad_id=VOCAB), f"{n}: top_p=1.500000 must be in (0, 1]"),
    ]
    for n in (SCALAR, PER_ROW):
        t += [
            (n, dict(advance=1, step=None), f"{n}: advance needs step"),
            (n, dict(pos_rows=-1), f"{n}: pos_rows=-1 must be >= 0"),
            (n, dict(unfinished=PTR, advance=1, step=None), f"{n}: unfinished needs finished"),
            (n, dict(advance=1, step=None, pos_rows=-1), f"{n}: advance needs step"),
        ]
    for n in (PER_ROW, SLOTS):
        need = f"{n}: temperature, top_k, top_p, seed and draw are required"
        t += [(n, {k: None}, need) for k in ARRAYS]
        t += [
            (n, dict(window=-1), f"{n}: window=-1 outside [0, 256]"),
            (n, dict(window=257), f"{n}: window=257 outside [0, 256]"),
            (n, dict(window=4), f"{n}: window=4 needs history"),
            (n, dict(max_length=PTR), f"{n}: max_length needs finished and length"),
            (n, dict(max_length=PTR, finished=PTR), f"{n}: max_length needs finished and length"),
            (n, dict(max_length=PTR, length=PTR), f"{n}: max_length needs finished and length"),
            (n, dict(draw=None, dtype=2), need),
            (n, dict(ld=VOCAB - 1, window=257), f"{n}: row stride below vocab"),
            (n, dict(window=257, max_length=PTR), f"{n}: window=257 outside [0, 256]"),
            (n, dict(window=4, max_length=PTR), f"{n}: window=4 needs history"),
            (n, dict(max_length=PTR, pad_id=VOCAB), f"{n}: max_length needs finished and length"),
        ]
    n = SLOTS
    t += [
        (n, dict(advance=1, pos=PTR, pos_rows=2), f"{n}: pos_rows=2 must be 0 or rows={ROWS}"),
        (n, dict(advance=1, pos=PTR, pos_rows=-1), f"{n}: pos_rows=-1 must be 0 or rows={ROWS}"),
        (n, dict(unfinished=PTR, advance=1, pos=PTR, pos_rows=2), f"{n}: unfinished needs finished"),
    ]
    return t


TABLE = _table()


def run(entry, fields):
    """The entry point on its base struct with `fields` overwritten (None: a
    null struct pointer).  Returns (status, message)."""
    from mtts import _lib
    lib = _lib.lib()
    fn = getattr(lib, "mtts_" + entry)
    if fields is None:
        rc = fn(None, None)
    else:
        assert fields, "a table row must make its struct invalid"
        a = _base(entry)
        for k, v in fields.items():
            assert any(k == f[0] for f in a._fields_), k
            setattr(a, k, v)
        rc = fn(C.byref(a), None)
    return rc, lib.mtts_last_error().decode()


def _id(row):
    entry, fields, _ = row
    if fields is None:
        return entry + "-null"
    return entry + "-" + ",".join(f"{k}={'ptr' if v == PTR else v}" for k, v in fields.items())


@pytest.mark.parametrize("row", TABLE, ids=[_id(r) for r in TABLE])
def test_invalid_arguments_are_refused_with_their_message(row):
    entry, fields, message = row
    rc, got = run(entry, fields)
    assert rc == EINVAL
    assert got == message


def test_table_covers_every_entry_point_and_its_two_fault_rows():
    for n in (SCALAR, PER_ROW, SLOTS):
        rows = [r for r in TABLE if r[0] == n]
        assert len(rows) >= 25
        assert sum(1 for r in rows if r[1] is not None and len(r[1]) >= 2) >= 4
    assert len({_id(r) for r in TABLE}) == len(TABLE)
