"""Sequences of calls on one context: what one call leaves in the context's scratch must not
reach the next. The fused path's scratch (csrc/b2f_fused.hip, fused_scratch_bytes) holds the
eval's half-round tile descriptors, and eval_desc_kernel writes none for a batch without
half-round tiles (every instance has 0 rounds): the fast pass must then read none, whatever an
earlier call left there -- the fused launch's counters (which aliased desc[0] through round 6), a
real descriptor of a larger batch, or uninitialised memory. Needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

from conftest import random_inputs
from verdict_util import INIT_ROWS, NONE, dev_flip

pytestmark = pytest.mark.gpu


def _eval(engine, batch):
    batch.evaluate(engine)
    path = engine.debug_eval_path()
    return path, batch.report_dict()


def _whole(orc, batch):
    adv, fixed = batch.host_trace()
    return orc.evaluate(adv, fixed, batch.offsets_host)


def _filled(engine, x):
    import b2f

    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    engine.sync(0)
    return batch


def _flagged(engine, orc, batch, col, row, mask):
    dev_flip(batch, col, row, mask)
    try:
        path, g = _eval(engine, batch)
        o = _whole(orc, batch)
    finally:
        dev_flip(batch, col, row, mask)
    assert o["first_failure"] != NONE, ("the oracle does not flag this flip", col, row)
    assert g == o and path == 1, (col, row, path, g, o)


def test_zero_round_evals_between_other_calls(engine, orc):
    import torch

    import b2f

    s = torch.cuda.current_stream().cuda_stream
    # 1. a fused call: its instance and edge-tile counters end up non-zero in the scratch
    x12 = random_inputs(300, (12,), 71)
    b12 = b2f.DeviceBatch(x12)
    b12.fill_evaluate(engine)
    engine.sync(s)
    assert b12.report_dict()["first_failure"] == NONE

    # 2. all-zero-round batches: no half-round tile, the fast pass is the edge walk alone
    zero = {}
    for n in (1, 9, 300):
        z = _filled(engine, random_inputs(n, (0,), 72 + n))
        assert z.total_rows == 228 * n
        path, rep = _eval(engine, z)
        assert path == 0, "the fast pass flagged a clean zero-round batch (n = %d)" % n
        assert rep == _whole(orc, z) and rep["first_failure"] == NONE
        assert rep["rows_checked"] == 228 * n
        zero[n] = z

    # 3. faults in the last instance's init and final regions
    z = zero[300]
    o299 = int(z.offsets_host[299])
    _flagged(engine, orc, z, 1, o299 + 57, 1 << 4)
    _flagged(engine, orc, z, 2, o299 + INIT_ROWS + 21, 1 << 9)
    path, rep = _eval(engine, z)
    assert path == 0 and rep["first_failure"] == NONE

    # 4. a split eval of the 12-round batch writes 7,200 real descriptors; the zero-round batch
    # after it must not decode descriptor 0 of that batch
    path, rep = _eval(engine, b12)
    assert path == 0 and rep["first_failure"] == NONE and rep["rows_checked"] == b12.total_rows
    path, rep = _eval(engine, zero[9])
    assert path == 0 and rep == _whole(orc, zero[9]) and rep["first_failure"] == NONE

    # 5. the only instance with half-rounds is the last one: tiles 0 .. 5 all belong to it
    xm = random_inputs(70, (0,), 75)
    xm["rounds"][-1] = 3
    m = _filled(engine, xm)
    path, rep = _eval(engine, m)
    assert path == 0 and rep == _whole(orc, m) and rep["first_failure"] == NONE
    _flagged(engine, orc, m, 4, int(m.offsets_host[69]) + INIT_ROWS + 30, 1 << 3)
    path, rep = _eval(engine, m)
    assert path == 0 and rep["first_failure"] == NONE
