"""Single-bit faults over every trace cell: the batches, the masks, the derived set of constrained
cells and the oracle's verdict per fault, shared by tests/test_cell_sweep_ref.py (CPU) and
tests/test_gpu_cell_sweep.py (the fast pass, the exact kernel and the fused pass).

A cell is (col, row): col 0..9 = a_col, 10 = the fixed column; row is the global row. A fault XORs
one bit into one cell of the clean trace. Which faults a correct checker rejects follows from the
constraint system alone (`constrained_cells`): the lookup runs on a_0, a_1, a_2 of every row, the
fixed column is pinned to keygen's on every row, a copy constraint pins both of its ends, and a
gate pins every cell it reads at a row where its selector is on. Every other cell is free, and
holds 0 in a clean trace.

  batch A  rounds [1, 2, 0, 1], 2,576 rows + 8 zero rows: three 1,024-row tiles of the exact
           kernel (the tile edge at row 1,024 inside the 2-round instance), a 0-round instance
           between two others. Every cell is swept; the cells of the 2-round instance with bits 0,
           15, 16 and 31 each (the cells are 16-bit limbs and spread forms, the fixed column's
           bits 16..31 are k_0: a checker that truncates before it compares misses the high
           ones), every other cell with one bit drawn per cell.
  batch B  rounds [12, 13, 0], 11,084 rows + 8 zero rows: 24 half-round tiles precede the 13-round
           instance, so it starts at a band start of the fast pass, owns a later segment of the
           fused pass (24 half-rounds per segment) and holds global row 8,192, the edge of the
           exact kernel's 8-tile band. Swept in windows: half-round tiles 23 and 24 of that
           instance, its 64 final rows, global rows 8,192 +- 104; one drawn bit per cell.
"""
import numpy as np

import quotient_gates_ref as gr
from verdict_util import FIXED_COL, INIT_ROWS, NONE, ROUND_ROWS

NCOLS = 11  # a_0 .. a_9 and the fixed column
FINAL_ROWS = 64
PAD_ROWS = 8
HIGH_LOW_BITS = (0, 15, 16, 31)
COUNTERS = ("gate_failures", "lookup_failures", "copy_failures", "fixed_failures")

_SPEC = {"A": dict(rounds=(1, 2, 0, 1), seed=71), "B": dict(rounds=(12, 13, 0), seed=72)}


def _orc():
    import oracle

    oracle.lib()
    return oracle


def gate_reads():
    """{selector bit: sorted (a_c, rotation) cells its polynomials read}, from the gate table of
    tests/quotient_gates_ref.py called with a recording accessor; bit 14 reads a_1@0."""
    out = {}
    for g in range(16):
        seen = set()

        def a(c, j):
            seen.add((c, j))
            return 0

        if g == 14:
            a(1, 0)
        else:
            gr.GATES[g](a)
        out[g] = sorted(seen)
    return out


def constrained_cells(rounds, total_rows):
    """bool [11, total_rows]: the cells a fault in which must be rejected, derived from the oracle's
    keygen fixed column, its copy constraints and the gates' reads. Runs no evaluation."""
    orc = _orc()
    rows = [INIT_ROWS + ROUND_ROWS * int(r) + FINAL_ROWS for r in rounds]
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)
    total = int(total_rows)
    assert total >= int(off[-1])
    fx = orc.fixed_structure(off, total)
    con = np.zeros((NCOLS, total), dtype=bool)
    con[0:3] = True  # the spread lookup: (a_0, a_1, a_2) of every row
    con[FIXED_COL] = True  # keygen's column on every row, zero past the instances
    for i, r in enumerate(rounds):
        base = int(off[i])
        for dr, dc, sr, sc in orc.copies(int(r)).astype(np.int64):
            con[dc, base + dr] = True
            con[sc, base + sr] = True
    for g, cells in gate_reads().items():
        on = np.flatnonzero((fx >> np.uint32(g)) & np.uint32(1))
        for c, j in cells:
            r = on + j
            con[c, r[r < total]] = True  # a gate's rows past the trace read no cell
    return con


class Batch:
    """One sweep batch: inputs, row map, the oracle's clean trace (host) and clean report, the
    constrained cells, the swept rows and the masks of every swept cell."""

    def __init__(self, name):
        from conftest import random_inputs

        orc = _orc()
        spec = _SPEC[name]
        self.name = name
        self.rounds = tuple(spec["rounds"])
        self.n = len(self.rounds)
        x = random_inputs(self.n, (0,), spec["seed"])
        x["rounds"] = np.asarray(self.rounds, dtype=np.uint32)
        self.inputs = x
        ox = np.frombuffer(x.tobytes(), dtype=orc.INPUT_DTYPE).copy()
        self.used = int(orc.offsets(ox)[-1])
        self.total = self.used + PAD_ROWS
        self.adv, self.fixed, self.h_out, off = orc.fill(ox, total_rows=self.total)
        self.off = off.astype(np.uint64)
        self.clean = orc.evaluate(self.adv, self.fixed, self.off, nthreads=1)
        assert self.clean["first_failure"] == NONE and self.clean["rows_checked"] == self.total
        self.constrained = constrained_cells(self.rounds, self.total)
        if name == "A":
            self.rows = np.arange(self.total)
            self.four = (int(self.off[1]), int(self.off[2]))  # the 2-round instance: four masks
        else:
            o = int(self.off[1])
            assert o == 24 * 208 + INIT_ROWS + FINAL_ROWS and o < 8192 - 104 and 8192 + 104 < int(self.off[2])
            hr = o + INIT_ROWS + 208 * 23
            fin = o + INIT_ROWS + ROUND_ROWS * 13
            self.rows = np.unique(np.concatenate([np.arange(hr, hr + 416), np.arange(fin, fin + 64),
                                                  np.arange(8192 - 104, 8192 + 104)]))
            self.four = (0, 0)
        # one bit per cell from a seeded generator, indexed by the cell itself: the copies of a role
        # (every 52 rows, every round) get unrelated bits
        self.bit = np.random.default_rng(1000 + spec["seed"]).integers(0, 32, (NCOLS, self.total))

    def instance_of(self, row):
        """The instance that holds `row`; the last one for the zero rows past the batch."""
        return min(int(np.searchsorted(self.off, row, side="right")) - 1, self.n - 1)

    def masks(self, col, row):
        if self.four[0] <= row < self.four[1]:
            return [1 << b for b in HIGH_LOW_BITS]
        return [1 << int(self.bit[col, row])]

    def cases(self, col):
        """[(row, mask)] of the swept cells of one column, in row order."""
        return [(int(r), m) for r in self.rows for m in self.masks(col, int(r))]

    def n_cases(self):
        """Swept (row, mask) pairs of one column (the same for every column)."""
        lo, hi = self.four
        return len(self.rows) + 3 * int(np.count_nonzero((self.rows >= lo) & (self.rows < hi)))

    def n_constrained_cases(self, col):
        return sum(len(self.masks(col, int(r))) for r in self.rows if self.constrained[col, r])


_batches = {}
_verdicts = {}


def batch(name):
    if name not in _batches:
        _batches[name] = Batch(name)
    return _batches[name]


def signed32(mask):
    """A 32-bit mask as the int32 value with that bit pattern (bit 31: negative), for the int32
    trace tensors."""
    mask = int(mask) & 0xffffffff
    return mask - (1 << 32) if mask >> 31 else mask


def dev_flip32(dev_batch, col, row, mask):
    """XOR any 32-bit `mask` into one cell of the device trace; twice restores it. (verdict_util's
    dev_flip takes masks below 2^31 only: the tensors are int32.)"""
    t = dev_batch.fixed if col == FIXED_COL else dev_batch.advice[col]
    t[int(row)] ^= signed32(mask)


def oracle_verdict(name, col, row, mask):
    """The oracle's report on batch `name`'s clean trace with `mask` XORed into cell (col, row),
    memoised: the three GPU checkers share one CPU evaluation per fault. For batch B the oracle
    runs on the instances around the fault only (the others are clean), re-based as
    verdict_util.oracle_window does: first_failure to the global row, rows_checked the batch's."""
    key = (name, int(col), int(row), int(mask))
    if key in _verdicts:
        return _verdicts[key]
    orc = _orc()
    b = batch(name)
    cell = b.fixed[row:row + 1] if col == FIXED_COL else b.adv[col, row:row + 1]
    cell ^= np.uint32(mask)
    try:
        if name == "A":
            o = orc.evaluate(b.adv, b.fixed, b.off, nthreads=1)
        else:
            i = b.instance_of(row)
            lo, hi = max(0, i - 1), min(b.n, i + 2)
            r0 = int(b.off[lo])
            r1 = b.total if hi == b.n else int(b.off[hi])
            o = orc.evaluate(b.adv[:, r0:r1], b.fixed[r0:r1], b.off[lo:hi + 1] - np.uint64(r0),
                             nthreads=1)
            if o["first_failure"] != NONE:
                o["first_failure"] += r0 << 8
            o["rows_checked"] = b.total
    finally:
        cell ^= np.uint32(mask)
    _verdicts[key] = o
    return o


def rejected(report):
    return report["first_failure"] != NONE


def counters_differ(report, clean):
    return any(report[k] != clean[k] for k in COUNTERS)
