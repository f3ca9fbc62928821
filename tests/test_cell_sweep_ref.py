"""tests/cell_sweep.py pinned on the CPU: the oracle rejects a single-bit fault exactly in the
constrained cells, the set derived from the constraint system (keygen's fixed column, the copy
constraints, the gates' reads) without running an evaluation.

Batch A (rounds [1, 2, 0, 1] + 8 zero rows, 28,424 cells) with bit 0 and with bit 31 in every cell,
batch B's windows (rounds [12, 13, 0]: two half-round tiles of the 13-round instance, its final
rows, rows 8,192 +- 104) with the sweep's one drawn bit per cell. For each: the set of rejected
cells equals constrained_cells, every free cell holds 0 in the clean trace, every rejected fault
moves a failure counter (not first_failure alone), a fault in a free cell leaves the whole report
as it was, and the cases evaluated are rows x 11. Batch A's counts are pinned: 14,164 constrained
and 14,260 free, the free ones 1,407 + 2,144 rounds per instance plus a_3..a_9 of the zero rows."""
import numpy as np
import pytest

import cell_sweep as cs


def _sweep(name, mask_of):
    """(rejected bool [11, rows], cases) over the swept rows of a batch; asserts the per-fault
    properties on the way."""
    b = cs.batch(name)
    rej = np.zeros((cs.NCOLS, len(b.rows)), dtype=bool)
    cases = 0
    for col in range(cs.NCOLS):
        for k, row in enumerate(b.rows):
            row = int(row)
            mask = mask_of(b, col, row)
            o = cs.oracle_verdict(name, col, row, mask)
            cases += 1
            rej[col, k] = cs.rejected(o)
            if rej[col, k]:
                assert cs.counters_differ(o, b.clean), (name, col, row, mask, o)
                assert o["rows_checked"] == b.total
                assert o["first_failure"] >> 8 < b.total
            else:
                assert o == b.clean, (name, col, row, mask, o)
    return b, rej, cases


def _check_sets(b, rej):
    want = b.constrained[:, b.rows]
    diff = np.argwhere(rej != want)
    assert diff.size == 0, "oracle and derived set differ at (col, row, oracle rejects): %s" % (
        [(int(c), int(b.rows[k]), bool(rej[c, k])) for c, k in diff[:20]],)
    clean = np.concatenate([b.adv, b.fixed[None, :]])[:, b.rows]
    assert not clean[~want].any(), "a free cell is not 0 in the clean trace"


@pytest.mark.parametrize("bit", [0, 31])
def test_batch_a_rejected_cells_are_the_constrained_cells(orc, bit):
    b, rej, cases = _sweep("A", lambda b, col, row: 1 << bit)
    assert b.total == 2584 and cases == 2584 * 11 == 28424
    _check_sets(b, rej)
    assert int(rej.sum()) == 14164 and int((~rej).sum()) == 14260
    for i, r in enumerate(b.rounds):
        lo, hi = int(b.off[i]), int(b.off[i + 1])
        assert int((~rej[:, lo:hi]).sum()) == 1407 + 2144 * r, (i, r)
    pad = ~rej[:, b.used:]
    assert pad.shape == (11, 8) and int(pad.sum()) == 56
    assert pad[3:10].all() and not pad[0:3].any() and not pad[10].any()


def test_batch_a_masks(orc):
    """The GPU sweep's masks of batch A: bits 0, 15, 16 and 31 in every cell of the 2-round
    instance, one drawn bit elsewhere, and the drawn bits do not repeat with the 52-row G period."""
    b = cs.batch("A")
    lo, hi = b.four
    assert hi - lo == 164 + 2 * 416 + 64 and lo < 1024 < hi
    assert b.n_cases() == 2584 + 3 * (hi - lo)
    for col in (0, 5, 10):
        got = b.cases(col)
        assert len(got) == b.n_cases()
        assert [m for r, m in got if r == 1024] == [1 << 0, 1 << 15, 1 << 16, 1 << 31]
        assert sum(1 for r, m in got if b.constrained[col, r]) == b.n_constrained_cases(col)
    # within a round, the eight G blocks' copies of one role draw different bits
    o = int(b.off[3]) + 164
    assert len({int(b.bit[4, o + 52 * g + 7]) for g in range(8)}) > 2
    assert set(np.unique(b.bit)) == set(range(32))
    assert cs.signed32(1 << 31) == -2**31 and cs.signed32(1 << 16) == 1 << 16


def test_batch_b_windows_rejected_cells_are_the_constrained_cells(orc):
    b, rej, cases = _sweep("B", lambda b, col, row: 1 << int(b.bit[col, row]))
    assert b.used == 11084 and b.total == 11092
    o = int(b.off[1])
    assert o == 5220 and (o - 228) // 208 == 24  # 24 half-round tiles precede the instance
    assert len(b.rows) == 416 + 64 + 208 and cases == len(b.rows) * 11
    assert {8192 - 104, 8192, 8192 + 103, o + 164 + 208 * 23, o + 164 + 208 * 25 - 1,
            int(b.off[2]) - 1} <= set(int(r) for r in b.rows)
    _check_sets(b, rej)
    # the window evaluation is the whole-trace evaluation (spot checks on both kinds of cell)
    for col, row in ((1, 8192), (6, 8190), (10, int(b.off[2]) - 3), (9, o + 164 + 208 * 24)):
        mask = 1 << int(b.bit[col, row])
        cell = b.fixed[row:row + 1] if col == 10 else b.adv[col, row:row + 1]
        cell ^= np.uint32(mask)
        try:
            whole = orc.evaluate(b.adv, b.fixed, b.off)
        finally:
            cell ^= np.uint32(mask)
        assert cs.oracle_verdict("B", col, row, mask) == whole, (col, row)
