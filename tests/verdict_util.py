"""Helpers shared by the GPU verdict tests on batches too large to round-trip per case: single
cells are flipped on the device, and the oracle runs on a window of instances around the fault
(the rest of the trace is known clean), re-based to the global row."""
import numpy as np

NONE = 2**64 - 1
INIT_ROWS, ROUND_ROWS, FINAL_ROWS = 164, 416, 64
FIXED_COL = 10  # column index of the fixed column in (column, row) fault coordinates


def dev_flip(batch, col, row, mask):
    """XOR `mask` (< 2^31) into one cell of the device trace; applying it twice restores it."""
    t = batch.fixed if col == FIXED_COL else batch.advice[col]
    t[int(row)] ^= int(mask)


def rounds_of(off, i):
    return int((int(off[i + 1]) - int(off[i]) - INIT_ROWS - FINAL_ROWS) // ROUND_ROWS)


def oracle_window(orc, batch, i):
    """The oracle's report on the device trace of instances i - 1 .. i + 1 (those that exist; for
    the last instance the zero rows past the batch too), as the report of the whole trace whose
    other instances are clean: first_failure re-based to the global row, rows_checked the
    batch's. Neighbours are included so a gate that reaches across an instance boundary reads
    what it reads in the whole trace."""
    off = batch.offsets_host
    a, b = max(0, i - 1), min(batch.n, i + 2)
    r0 = int(off[a])
    r1 = batch.total_rows if b == batch.n else int(off[b])
    adv = batch.advice[:, r0:r1].cpu().numpy().view(np.uint32)
    fx = batch.fixed[r0:r1].cpu().numpy().view(np.uint32)
    sub = (off[a:b + 1].astype(np.uint64) - np.uint64(r0)).astype(np.uint64)
    o = orc.evaluate(adv, fx, sub)
    if o["first_failure"] != NONE:
        o["first_failure"] += r0 << 8
    o["rows_checked"] = batch.total_rows
    return o
