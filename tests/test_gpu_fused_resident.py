"""GPU checks of the fused pass's advice-only launch (b2f_fill_eval_dev_ex with
B2F_FIXED_RESIDENT, csrc/b2f_fused.hip FZ_NOFIX): a repeat call on the same row map and buffers
leaves the fixed column -- keygen output, a function of the row map alone -- in place.

What must hold: the advice-only launch stores nothing to the fixed column (not from the
half-round tiles, the boundary edge tiles or the zero rows past the batch) and writes the same
advice, h' and report as the split path (b2f_fill_dev + b2f_eval_dev); the library honours the
flag only against its own record of the last full write; DeviceBatch states it only while its
seal (engine context, version counters of `fixed` and `offsets`) holds; and a call under the
inject hook always runs in full. The shapes are the junction shapes of test_gpu_fused_lines.py,
not the workload's. Every test here needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

from conftest import random_inputs
from verdict_util import INIT_ROWS, NONE

pytestmark = pytest.mark.gpu

ROUNDS = [0, 1, 0, 0, 2, 12, 13, 1, 0, 4, 25, 0]  # 13 and 25: a listed segment in every case
ROTATED = ROUNDS[5:] + ROUNDS[:5]
ORDERS = {"zero_first": ROUNDS + ROTATED, "zero_last": ROTATED + ROUNDS}
# total_rows = used + pad: the columns at different line offsets; 552 rows past the batch are two
# full zero-row tiles (64 quads each) and a partial one
PADS = [0, 4, 20, 552]
POISON = -0x21524111  # 0xdeadbeef as int32
RESIDENT = 1  # B2F_FIXED_RESIDENT


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _inputs(rounds, seed):
    x = random_inputs(len(rounds), (12,), seed)
    x["rounds"] = np.asarray(rounds, dtype=np.uint32)
    return x


def _poison(batch, fixed=True):
    batch.advice.fill_(POISON)
    if fixed:
        batch.fixed.fill_(POISON)
    batch.h_out.fill_(-1)
    batch.report.fill_(-1)


_SPLIT = {}


def _case(engine, order, pad):
    """(inputs, total_rows, the split path's batch over poisoned buffers, its report), computed
    once per shape and left unchanged."""
    import b2f

    key = (order, pad)
    if key not in _SPLIT:
        x = _inputs(ORDERS[order], 170 + pad)
        total = int(b2f.offsets(x)[-1]) + pad
        _SPLIT[key] = (x, total) + _split(engine, x, total)
    return _SPLIT[key]


def _split(engine, x, total):
    """The split path's batch over poisoned buffers and its report."""
    import b2f

    batch = b2f.DeviceBatch(x, total_rows=total)
    _poison(batch)
    batch.fill(engine)
    batch.evaluate(engine)
    engine.sync(_stream())
    rep = batch.report_dict()
    assert rep["first_failure"] == NONE
    return batch, rep


def _call(eng, batch, flags, total_rows=None):
    """The engine-level fused call on the batch's buffers."""
    eng.fill_eval_dev(batch.inputs.data_ptr(), batch.n, batch.offsets.data_ptr(),
                      batch.total_rows if total_rows is None else total_rows,
                      batch.advice.data_ptr(), batch.fixed.data_ptr(), batch.h_out.data_ptr(),
                      batch.report.data_ptr(), _stream(), flags=flags)


def _assert_outputs(batch, split, want, fixed=True):
    import torch

    for c in range(10):
        bad = (batch.advice[c] != split.advice[c]).nonzero().reshape(-1).tolist()
        assert bad == [], "a_%d differs at rows %s" % (c, bad[:10])
    if fixed:
        assert torch.equal(batch.fixed, split.fixed)
    assert torch.equal(batch.h_out, split.h_out)
    assert batch.report_dict() == want


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("pad", PADS)
def test_resident_call_stores_nothing_to_fixed(engine, order, pad):
    """After a full call, B2F_FIXED_RESIDENT on the same pointers runs the advice-only launch:
    every word of a `fixed` overwritten with a sentinel is still the sentinel (half-round tiles,
    boundary tiles at both ends and inside runs of 0-round instances, zero rows), while the
    poisoned advice, h' and report come back equal to the split path's bit for bit."""
    import b2f

    x, total, split, want = _case(engine, order, pad)
    batch = b2f.DeviceBatch(x, total_rows=total)
    _poison(batch)
    _call(engine, batch, 0)
    assert engine.debug_fused_path() == 0
    engine.sync(_stream())
    _assert_outputs(batch, split, want)
    _poison(batch)
    _call(engine, batch, RESIDENT)
    assert engine.debug_fused_path() == 1
    engine.sync(_stream())
    left = (batch.fixed != POISON).nonzero().reshape(-1).tolist()
    assert left == [], "fixed written at rows %s" % left[:10]
    _assert_outputs(batch, split, want, fixed=False)


def test_library_guard_refuses_an_unrecorded_column(engine):
    """The flag alone does not make the column resident: on a fresh context, after a full call
    on other buffers, and on the recorded buffers with another total_rows, the call runs in
    full (path 0) and restores a poisoned `fixed`."""
    import b2f
    import torch

    x, total, split, want = _case(engine, "zero_first", 20)
    batch = b2f.DeviceBatch(x, total_rows=total)
    fresh = b2f.Engine(0)
    try:
        _poison(batch)
        _call(fresh, batch, RESIDENT)
        assert fresh.debug_fused_path() == 0
        fresh.sync(_stream())
        _assert_outputs(batch, split, want)
    finally:
        fresh.close()
    # the session engine's record names another batch's buffers
    other = b2f.DeviceBatch(x, total_rows=total)
    _call(engine, other, 0)
    _poison(batch)
    _call(engine, batch, RESIDENT)
    assert engine.debug_fused_path() == 0
    engine.sync(_stream())
    _assert_outputs(batch, split, want)
    # the record now names this batch's buffers at `total` rows: the same buffers as a trace of
    # total - 16 rows (columns at another stride) is another column
    total4 = total - 16
    split4, want4 = _split(engine, x, total4)
    _poison(batch)
    _call(engine, batch, RESIDENT, total_rows=total4)
    assert engine.debug_fused_path() == 0
    engine.sync(_stream())
    adv = batch.advice.reshape(-1)[:10 * total4].reshape(10, total4)
    assert torch.equal(adv, split4.advice)
    assert torch.equal(batch.fixed[:total4], split4.fixed)
    assert torch.equal(batch.h_out, split4.h_out) and batch.report_dict() == want4
    # ... and that full call renewed the record for total4
    _call(engine, batch, RESIDENT, total_rows=total4)
    assert engine.debug_fused_path() == 1
    engine.sync(_stream())


def test_device_batch_sequence(engine, diag_engine):
    """DeviceBatch.fill_evaluate decides by its seal: first call full, repeat advice-only; a
    torch write to `fixed`, fixed_resident=False, a call on the diagnostics engine and
    invalidate_fixed() each make the next call full, and the trace is whole after every call."""
    import b2f

    x, total, split, want = _case(engine, "zero_last", 4)
    batch = b2f.DeviceBatch(x, total_rows=total)

    def step(path, eng=engine, **kw):
        batch.advice.fill_(POISON)
        batch.h_out.fill_(-1)
        batch.fill_evaluate(eng, **kw)
        if path is not None:
            assert eng.debug_fused_path() == path
        eng.sync(_stream())
        _assert_outputs(batch, split, want)

    _poison(batch)
    step(0)
    step(1)
    batch.fixed.fill_(POISON)
    step(0)
    step(1)
    step(0, fixed_resident=False)
    step(1)
    batch.fixed.fill_(POISON)
    step(0, eng=diag_engine)  # the diagnostics build never leaves the column out
    step(0)
    step(1)
    batch.invalidate_fixed()
    step(0)
    step(1)


# a_1 is the spread lookup's dense column, read on every row, so a flipped bit there is a
# failure wherever the row is (a_3 .. a_9 hold cells no gate reads at many rows of a tile: the
# standalone eval passes a flip there too); 10 is the fixed column
@pytest.mark.parametrize("col", [1, 10])
@pytest.mark.parametrize("where", ["junction", "mid_tile"])
def test_inject_hook_runs_full_and_clears_the_record(engine, col, where):
    """Under b2f_debug_inject a sealed batch's call still runs in full: the written trace is the
    clean one with exactly the injected cell flipped (a fixed cell too), and the report is
    b2f_eval_dev's on that trace. With the hook off the next call is full again -- the hook's
    call may have left a faulted fixed cell -- and restores the keygen column; the one after
    is advice-only."""
    import b2f
    import torch

    x, total, split, want = _case(engine, "zero_first", 20)
    i = 5  # the 12-round instance
    assert ORDERS["zero_first"][i] == 12
    o = int(split.offsets_host[i])
    # the first row of the first half-round tile (its line is shared with the init region), or a
    # row inside the fourth tile
    row = o + INIT_ROWS if where == "junction" else o + INIT_ROWS + 3 * 208 + 101
    mask = 1 << 9
    batch = b2f.DeviceBatch(x, total_rows=total)
    batch.fill_evaluate(engine)
    batch.fill_evaluate(engine)
    assert engine.debug_fused_path() == 1
    _poison(batch, fixed=False)
    try:
        engine.debug_inject(row, col, mask)
        batch.fill_evaluate(engine)
        assert engine.debug_fused_path() == 0
        engine.sync(_stream())
    finally:
        engine.debug_inject(None)
    got = batch.report_dict()
    diff_a = (batch.advice != split.advice).nonzero().tolist()
    diff_f = (batch.fixed != split.fixed).nonzero().reshape(-1).tolist()
    assert (diff_a, diff_f) == (([[col, row]], []) if col < 10 else ([], [row]))
    cell = batch.advice[col, row] if col < 10 else batch.fixed[row]
    ref_cell = split.advice[col, row] if col < 10 else split.fixed[row]
    assert int(cell) ^ int(ref_cell) == mask
    assert torch.equal(batch.h_out, split.h_out)
    batch.evaluate(engine)  # the standalone eval on the written trace
    engine.sync(_stream())
    assert got == batch.report_dict()
    assert got["first_failure"] != NONE
    # hook off: full, and the column is keygen's again
    keygen = torch.full_like(batch.fixed, POISON)
    engine.fill_fixed_dev(batch.offsets.data_ptr(), batch.n, total, keygen.data_ptr(), _stream())
    batch.fill_evaluate(engine)
    assert engine.debug_fused_path() == 0
    engine.sync(_stream())
    assert torch.equal(batch.fixed, keygen)
    _assert_outputs(batch, split, want)
    batch.fill_evaluate(engine)
    assert engine.debug_fused_path() == 1
    engine.sync(_stream())
    _assert_outputs(batch, split, want)


def test_benchmark_order_third_call_equals_a_fresh_full_call(engine):
    """The benchmark's own sequence at a small size: one batch, fill_evaluate step after step.
    The third call's advice, fixed, h' and report equal a fresh batch's single full call."""
    import b2f
    import torch
    from b2f import synth

    x = synth.batch(4096, rounds_mix=[1, 4, 12])
    batch = b2f.DeviceBatch(x)
    _poison(batch)
    paths = []
    for _ in range(3):
        batch.advice.fill_(POISON)
        batch.h_out.fill_(-1)
        batch.fill_evaluate(engine)
        paths.append(engine.debug_fused_path())
    engine.sync(_stream())
    assert paths == [0, 1, 1]
    fresh = b2f.DeviceBatch(x)
    _poison(fresh)
    fresh.fill_evaluate(engine, fixed_resident=False)
    assert engine.debug_fused_path() == 0
    engine.sync(_stream())
    assert fresh.report_dict()["first_failure"] == NONE
    assert torch.equal(batch.advice, fresh.advice)
    assert torch.equal(batch.fixed, fresh.fixed)
    assert torch.equal(batch.h_out, fresh.h_out)
    assert batch.report_dict() == fresh.report_dict()
