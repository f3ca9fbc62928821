"""GPU checks of the fused pass's stores at the junctions of an instance's regions
(csrc/b2f_fused.hip): init | first half-round, last half-round | final, final | next init.

An edge tile of the fused launch is an instance BOUNDARY: the final region of instance b - 1
and the init region of instance b, adjacent in memory, staged by one wave and stored as one
contiguous run per column, so the 128-byte line the two regions share is written once. The run
begins and ends on a line: an instance's first half-round tile forms and stores the init quads
of its first line (kc of them), and its last tile leaves the quads of its last line (tc) to the
boundary tile, which recomputes them. The tile's two regions belong to two instances, so a
flagged instance is re-checked exactly region by region, each region by the one boundary tile
that holds it.

What must hold whatever the junctions do: the fused trace (advice, fixed, the zero rows past the
batch), h' and the report equal the split path's (b2f_fill_dev + b2f_eval_dev) bit for bit at
every line offset of every column, and a fault injected at a junction appears in the written
trace exactly once and is counted exactly once. Every test here needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

from conftest import random_inputs
from verdict_util import INIT_ROWS, NONE, ROUND_ROWS

pytestmark = pytest.mark.gpu

ROUNDS = [0, 1, 0, 0, 2, 12, 13, 1, 0, 4, 25, 0]  # 13 and 25: a listed segment in every case
ROTATED = ROUNDS[5:] + ROUNDS[:5]
POISON = -0x21524111  # 0xdeadbeef as int32


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _inputs(rounds, seed):
    x = random_inputs(len(rounds), (12,), seed)
    x["rounds"] = np.asarray(rounds, dtype=np.uint32)
    return x


def _poison(batch):
    batch.advice.fill_(POISON)
    batch.fixed.fill_(POISON)
    batch.h_out.fill_(-1)


def _split(engine, x, total_rows):
    """The split path's trace, h' and report over poisoned buffers."""
    import b2f

    batch = b2f.DeviceBatch(x, total_rows=total_rows)
    _poison(batch)
    batch.fill(engine)
    batch.evaluate(engine)
    engine.sync(_stream())
    return batch, batch.report_dict()


# 0-round instances first (ROUNDS + ROTATED) and last (ROTATED + ROUNDS)
@pytest.mark.parametrize("order", ["zero_first", "zero_last"])
@pytest.mark.parametrize("pad", [0, 4, 8, 12, 16, 20, 24, 28])
def test_fused_equals_split_at_every_line_offset(engine, order, pad):
    """Column c's line offset at a row is (c total_rows + row) mod 32 rows, so total_rows = used
    + 0, 4 .. 28 puts every column at every 16-byte offset of a line at every junction: the quads
    a half-round tile takes from (kc) or leaves to (tc) its neighbour take all of 0..7. Runs of
    0-round instances (init | final adjacent, no half-round tile), the first and the last
    instance, and total_rows == used_rows are the corners."""
    import b2f
    import torch

    rounds = ROUNDS + ROTATED if order == "zero_first" else ROTATED + ROUNDS
    assert rounds[0 if order == "zero_first" else -1] == 0
    x = _inputs(rounds, 70 + pad)
    total = int(b2f.offsets(x)[-1]) + pad
    split, want = _split(engine, x, total)
    assert want["first_failure"] == NONE
    fused = b2f.DeviceBatch(x, total_rows=total)
    _poison(fused)
    fused.fill_evaluate(engine)
    engine.sync(_stream())
    for c in range(10):
        bad = (fused.advice[c] != split.advice[c]).nonzero().reshape(-1).tolist()
        assert bad == [], "pad %d: a_%d differs at rows %s" % (pad, c, bad[:10])
    assert torch.equal(fused.fixed, split.fixed)
    assert torch.equal(fused.h_out, split.h_out)
    assert fused.report_dict() == want


# first and last instance with rounds, a 1-round instance between a 2-round and a 0-round one, a
# 0-round instance inside a run of them
JROUNDS = ROTATED + ROUNDS[1:] + [2]
JUNCTION_CASES = {"first": 0, "middle_1_round": 12, "middle_0_rounds": 9, "last": len(JROUNDS) - 1}


def _junction_rows(off, rounds, i, n):
    """Rows of instance i at its junctions (and of the next instance's first init quad)."""
    o, r = int(off[i]), int(rounds[i])
    quads = [o + 4 * q for q in range(33, 41)]  # init quads 33-40
    for h in ([0, 2 * r - 1] if r else []):  # first and last half-round tile
        t = o + INIT_ROWS + 208 * h
        quads += [t, t + 4, t + 4 * 50, t + 4 * 51]
    row_f = o + INIT_ROWS + ROUND_ROWS * r
    quads += [row_f + 4 * q for q in (0, 1, 2, 3, 4, 5, 6, 7, 15)]
    if i + 1 < n:
        quads.append(int(off[i + 1]))
    return sorted({q + j for q in quads for j in range(4)})


@pytest.mark.parametrize("where", sorted(JUNCTION_CASES))
def test_junction_faults_are_written_and_counted_once(engine, where):
    """One bit flipped (b2f_debug_inject) in every column at every row around the junctions of
    an instance: the fused report -- every counter and first_failure -- equals b2f_eval_dev's on
    the trace the fused call wrote (an instance flagged from both boundary tiles and re-checked
    twice would double a counter), and that trace is the split trace with exactly the injected
    bit flipped (a junction line written by two owners would carry the fault twice or not at
    all)."""
    import b2f
    import torch

    i = JUNCTION_CASES[where]
    x = _inputs(JROUNDS, 81)
    assert JROUNDS[0] > 0 and JROUNDS[-1] > 0 and JROUNDS[12] == 1 and JROUNDS[13] == 0
    assert JROUNDS[9] == 0 and JROUNDS[10] == 0
    total = int(b2f.offsets(x)[-1]) + 12
    split, clean = _split(engine, x, total)
    assert clean["first_failure"] == NONE
    want_adv, want_fix = split.advice, split.fixed  # faulted and restored cell by cell
    off = split.offsets_host
    fused = b2f.DeviceBatch(x, total_rows=total)
    flagged = cases = 0
    for row in _junction_rows(off, JROUNDS, i, len(JROUNDS)):
        for col in range(11):
            mask = 1 << ((5 * cases + col) % 32)
            mask32 = mask - (1 << 32) if mask >> 31 else mask
            cell = want_adv[col, row:row + 1] if col < 10 else want_fix[row:row + 1]
            _poison(fused)
            try:
                engine.debug_inject(row, col, mask)
                fused.fill_evaluate(engine)
                engine.sync(_stream())
            finally:
                engine.debug_inject(None)
            got = fused.report_dict()
            cell ^= mask32
            try:
                same = torch.equal(fused.advice, want_adv) and torch.equal(fused.fixed, want_fix)
            finally:
                cell ^= mask32
            assert same, "row %d (instance %d + %d) col %d: written trace != split ^ mask" % (
                row, i, row - int(off[i]), col)
            assert torch.equal(fused.h_out, split.h_out)
            fused.evaluate(engine)  # the standalone eval on the written trace
            engine.sync(_stream())
            ref = fused.report_dict()
            assert got == ref, (row - int(off[i]), col, mask, got, ref)
            flagged += got["first_failure"] != NONE
            cases += 1
    assert 3 * flagged >= cases, (flagged, cases)
