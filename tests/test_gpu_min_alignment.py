"""GPU checks of the witness and export calls on pointers that are 16-byte aligned and no more,
with poisoned guard bands around every buffer (tests/arena.py).

include/b2f.h promises b2f_fill_dev, b2f_eval_dev, b2f_fill_eval_dev[_ex], b2f_fill_fixed_dev and
the three export calls work at 16-byte alignment. The fused pass (csrc/b2f_fused.hip) is the one
kernel whose control flow depends on the address itself: a half-round tile takes, per column, the
quads it stores in front of itself (kc) and the quads it leaves to what follows (tc) from the low
bits of the real store address, and the boundary tile repeats that arithmetic from the other
side. With whole allocations as buffers the advice base, the fixed base and the row-derived bits
always agree modulo 128, so a tile that took the fixed column's kc from the advice base, or a
hand-off computed from the address on one side and from the row on the other, would pass every
other test; and nothing else reads the memory around a buffer, where a run that starts early or
ends late would land.

Here every buffer is carved from one poisoned arena at a chosen address modulo 128, the advice
and the fixed column at all 64 pairs of phases. The reference is the CPU oracle everywhere
(oracle.fill / evaluate / fixed_structure / export_fp, quotient_gates_ref.unpack_fixed with
ntt_ref.pack, lookup.tag / spread), never the same call on aligned buffers; one oracle result
per (rounds, total_rows) serves every phase, since the trace does not depend on where it lies.
All comparisons are bit-exact. The split kernels and the exports are address-blind; they get the
same two checks, least alignment and nothing written outside the buffer.

Not covered yet: the prover-column calls (NTT, lookup, permutation, quotient, opening, MSM, IPA,
group NTT) at least alignment. Every test here needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

import arena
from conftest import random_inputs
from test_gpu_fused_lines import JROUNDS, JUNCTION_CASES, ROTATED, ROUNDS, _junction_rows
from verdict_util import FINAL_ROWS, INIT_ROWS, NONE, ROUND_ROWS

pytestmark = pytest.mark.gpu

PHASES = list(range(0, 128, 16))
RESIDENT = 1  # B2F_FIXED_RESIDENT
ERR_ARG = 1
# the 24 instances of test_gpu_fused_lines.py (53,728 rows: runs of 0-round instances, 13- and
# 25-round instances with a listed segment each, the first and the last instance with and without
# rounds), a single 0-round and a single 1-round instance (228 and 644 rows), and the junction
# batch of test_junction_faults_are_written_and_counted_once: (rounds, seed)
BATCHES = {"lines24": (ROUNDS + ROTATED, 70), "one_0": ([0], 71), "one_1": ([1], 72),
           "junction": (JROUNDS, 81)}


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Case:
    """One (batch, total_rows): the inputs, the oracle's trace, h' and report on the host, and
    their uploads. Computed once, shared by every phase, never written."""


_CASES = {}


def _case(orc, name, pad):
    import torch

    key = (name, pad)
    if key in _CASES:
        return _CASES[key]
    rounds, seed = BATCHES[name]
    x = random_inputs(len(rounds), (12,), seed)
    x["rounds"] = np.asarray(rounds, dtype=np.uint32)
    c = Case()
    c.name, c.pad, c.n, c.rounds = name, pad, len(rounds), list(rounds)
    ox = np.frombuffer(x.tobytes(), dtype=orc.INPUT_DTYPE).copy()
    c.off = orc.offsets(ox)
    c.used = int(c.off[-1])
    c.total = c.used + pad
    c.adv, c.fixed, c.h, _ = orc.fill(ox, c.total)
    assert not c.adv[:, c.used:].any() and not c.fixed[c.used:].any()  # the oracle's pad rows
    assert np.array_equal(c.fixed, orc.fixed_structure(c.off, c.total))
    c.report = orc.evaluate(c.adv, c.fixed, c.off)
    assert c.report["first_failure"] == NONE and c.report["rows_checked"] == c.total
    dev = "cuda:0"
    c.d_in = torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.uint8).copy()).to(dev)
    c.d_off = torch.from_numpy(c.off.view(np.int64).copy()).to(dev)
    c.d_adv = torch.from_numpy(c.adv.view(np.int32).copy()).to(dev)
    c.d_fixed = torch.from_numpy(c.fixed.view(np.int32).copy()).to(dev)
    c.d_h = torch.from_numpy(c.h.view(np.int64).copy()).to(dev)
    _CASES[key] = c
    return c


class Bufs:
    """The six buffers of a trace call, each carved at its own phase; the inputs and the row map
    are copied in, the rest is poison."""

    def __init__(self, A, c, adv, fix, inp=0, h=0, rep=0, off=8):
        import b2f
        import torch

        self.inputs = A.carve(216 * c.n, inp, torch.uint8, "inputs")
        self.offsets = A.carve(8 * (c.n + 1), off, torch.int64, "offsets")
        self.advice = A.carve(40 * c.total, adv, name="advice").view(10, c.total)
        self.fixed = A.carve(4 * c.total, fix, name="fixed")
        self.h_out = A.carve(64 * c.n, h, torch.int64, "h_out").view(c.n, 8)
        self.report = A.carve(b2f._lib.REPORT_BYTES, rep, torch.int64, "report")
        self.inputs.copy_(c.d_in)
        self.offsets.copy_(c.d_off)
        assert self.advice.data_ptr() % 128 == adv and self.fixed.data_ptr() % 128 == fix
        assert self.offsets.data_ptr() % 16 == off % 16

    def report_dict(self):
        import b2f

        return b2f.EvalReport.from_buffer_copy(self.report.cpu().numpy().tobytes()).as_dict()

    def outputs(self):
        return (("advice", self.advice), ("fixed", self.fixed), ("h_out", self.h_out), ("report", self.report))


def _fused(engine, b, c, flags=0):
    engine.fill_eval_dev(b.inputs.data_ptr(), c.n, b.offsets.data_ptr(), c.total, b.advice.data_ptr(),
                         b.fixed.data_ptr(), b.h_out.data_ptr(), b.report.data_ptr(), _stream(), flags=flags)


def _fill(engine, b, c):
    engine.fill_dev(b.inputs.data_ptr(), c.n, b.offsets.data_ptr(), c.total, b.advice.data_ptr(),
                    b.fixed.data_ptr(), b.h_out.data_ptr(), _stream())


def _eval(engine, b, c):
    engine.eval_dev(b.advice.data_ptr(), b.fixed.data_ptr(), b.offsets.data_ptr(), c.n, c.total,
                    b.report.data_ptr(), _stream())


def _rows(t):
    bad = t.nonzero().reshape(-1).tolist()
    return "%d rows, first %s" % (len(bad), bad[:8])


def _assert_trace(b, c, what, advice=True, fixed=True, h=True):
    """The carved trace equals the oracle's, the rows past the batch are zero; a failure names the
    column, the rows and `what` (the phases)."""
    import torch

    if advice and not torch.equal(b.advice, c.d_adv):
        for col in range(10):
            diff = b.advice[col] != c.d_adv[col]
            assert not bool(diff.any()), "%s: a_%d differs from the oracle at %s" % (what, col, _rows(diff))
    if fixed and not torch.equal(b.fixed, c.d_fixed):
        diff = b.fixed != c.d_fixed
        assert False, "%s: the fixed column differs from the oracle at %s" % (what, _rows(diff))
    if c.total > c.used:
        for col in range(10 if advice else 0):
            tail = b.advice[col, c.used:]
            assert not bool(tail.any()), "%s: a_%d past the batch is not zero at %s (+ %d)" % (
                what, col, _rows(tail), c.used)
        if fixed:
            assert not bool(b.fixed[c.used:].any()), "%s: fixed past the batch is not zero" % what
    if h:
        assert torch.equal(b.h_out, c.d_h), "%s: h' differs from the oracle" % what


def _assert_guards(A, what):
    msg = A.first_dirty()
    assert msg is None, "%s: %s" % (what, msg)


# ---------------------------------------------------------------------------------------------
# 1. the fused pass at every pair of phases


def _pair_phases(ia, jf):
    """The phases of the other pointers, moving with the pair: each takes all eight residues over
    the 64 pairs; the row map's is 8 bytes past a 16-byte boundary."""
    return {"inp": 16 * ((ia + 3 * jf + 1) % 8), "h": 16 * ((3 * ia + jf + 2) % 8),
            "rep": 16 * ((5 * ia + 7 * jf + 5) % 8), "off": 8 + 16 * ((ia + jf) % 8)}


@pytest.mark.parametrize("pad", [0, 12, 1028])
@pytest.mark.parametrize("name", ["lines24", "one_0", "one_1"])
def test_fused_at_every_phase_pair(engine, orc, name, pad):
    """total_rows = used + 0 and used + 12: all 64 pairs (advice phase, fixed phase), the fixed
    column out of step with a_0 in 56 of them, the address bits out of step with the row bits
    wherever the phase is not 0. used + 1028 (several tiles of zero rows past the batch): the
    eight pairs with fixed = advice + 48. Everything is poison before the call; afterwards advice,
    fixed, h' and the report are the oracle's, the rows past the batch zero, and every byte
    between and around the buffers still poison."""
    c = _case(orc, name, pad)
    A = arena.shared()
    pairs = [(ia, jf) for ia in range(8) for jf in range(8)] if pad != 1028 else \
        [(ia, (ia + 3) % 8) for ia in range(8)]
    seen = {k: set() for k in ("advice", "fixed", "diff", "inputs", "h_out", "report", "offsets")}
    for ia, jf in pairs:
        what = "%s, total_rows = used + %d, advice phase %d, fixed phase %d" % (name, pad, 16 * ia, 16 * jf)
        A.reset()
        b = Bufs(A, c, 16 * ia, 16 * jf, **_pair_phases(ia, jf))
        _fused(engine, b, c)
        assert engine.debug_fused_path() == 0
        engine.sync(_stream())
        _assert_trace(b, c, what)
        assert b.report_dict() == c.report, what
        _assert_guards(A, what)
        pa, pf = b.advice.data_ptr() % 128, b.fixed.data_ptr() % 128
        seen["advice"].add(pa)
        seen["fixed"].add(pf)
        seen["diff"].add((pf - pa) % 128)
        seen["inputs"].add(b.inputs.data_ptr() % 128)
        seen["h_out"].add(b.h_out.data_ptr() % 128)
        seen["report"].add(b.report.data_ptr() % 128)
        seen["offsets"].add(b.offsets.data_ptr() % 128)
    # read from the pointers the calls were given, not from the phases asked for
    assert seen["advice"] == set(PHASES) and seen["fixed"] == set(PHASES)
    if pad != 1028:
        assert seen["diff"] == set(PHASES)  # all eight relative phases of fixed to advice
        assert seen["inputs"] == set(PHASES) and seen["h_out"] == set(PHASES) and seen["report"] == set(PHASES)
        assert seen["offsets"] == {p + 8 for p in PHASES}  # 8-byte aligned, never 16
    else:
        assert seen["diff"] == {48}


# ---------------------------------------------------------------------------------------------
# 2. the advice-only kernel (B2F_FIXED_RESIDENT)


@pytest.mark.parametrize("pad", [12, 1028])
def test_fused_advice_only_at_unequal_phases(engine, orc, pad):
    """A full call, then the advice alone poisoned and a B2F_FIXED_RESIDENT call on the same
    pointers: the advice-only kernel runs (its kc / tc come from the advice base alone), rewrites
    the advice to the oracle's, leaves the fixed column the oracle's, and reports the same."""
    c = _case(orc, "lines24", pad)
    A = arena.shared()
    for i in range(8):
        pa, pf = 16 * i, 16 * ((3 * i + 1) % 8)  # never equal; fixed - advice = 16, 48, 80, 112
        assert pa != pf
        what = "total_rows = used + %d, advice phase %d, fixed phase %d" % (pad, pa, pf)
        A.reset()
        b = Bufs(A, c, pa, pf, **_pair_phases(i, (3 * i + 1) % 8))
        _fused(engine, b, c)
        assert engine.debug_fused_path() == 0
        engine.sync(_stream())
        _assert_trace(b, c, what + ", full call")
        assert b.report_dict() == c.report, what
        for t in (b.advice, b.h_out, b.report):
            A.repoison(t)
        _fused(engine, b, c, RESIDENT)
        assert engine.debug_fused_path() == 1, what
        engine.sync(_stream())
        _assert_trace(b, c, what + ", advice-only call")
        assert b.report_dict() == c.report, what
        _assert_guards(A, what)


# ---------------------------------------------------------------------------------------------
# 3. a fault at a junction, written once and counted once


_JUNCTION = {}


def _junction_verdicts(orc, c):
    """(row, col, mask, the oracle's report on its trace with that bit flipped) for every column at
    every junction row of the 1-round instance between a 2-round and a 0-round one, the masks of
    test_junction_faults_are_written_and_counted_once. Computed once for both phase pairs."""
    if not _JUNCTION:
        i = JUNCTION_CASES["middle_1_round"]
        assert JROUNDS[i] == 1 and JROUNDS[i - 1] == 2 and JROUNDS[i + 1] == 0
        adv, fixed = c.adv.copy(), c.fixed.copy()
        out = []
        for row in _junction_rows(c.off, JROUNDS, i, len(JROUNDS)):
            for col in range(11):
                mask = 1 << ((5 * len(out) + col) % 32)
                cell = fixed[row:row + 1] if col == 10 else adv[col, row:row + 1]
                cell ^= np.uint32(mask)
                rep = orc.evaluate(adv, fixed, c.off)
                cell ^= np.uint32(mask)
                out.append((row, col, mask, rep))
        assert np.array_equal(adv, c.adv) and np.array_equal(fixed, c.fixed)
        _JUNCTION["cases"] = out
    return _JUNCTION["cases"]


@pytest.mark.parametrize("pa,pf", [(16, 80), (112, 32)])
def test_junction_fault_written_once_counted_once(engine, orc, pa, pf):
    """One bit flipped (b2f_debug_inject) in each of the eleven columns at each of the 104 junction
    rows, with the buffers at 16-byte-only addresses: the written trace is the oracle's with
    exactly that bit flipped (a junction line with two owners would carry it twice or not at
    all), the report is oracle.evaluate's on that trace (an instance flagged from both boundary
    tiles would double a counter), and the guards are whole. The oracle alone flags 578 of these
    1,144 faults (50.5 %, found on the CPU before any GPU run): the closing condition of the
    test this one follows, a third at least, holds with room."""
    import torch

    c = _case(orc, "junction", 12)
    cases = _junction_verdicts(orc, c)
    assert len(cases) == 11 * 104
    assert 3 * sum(rep["first_failure"] != NONE for _, _, _, rep in cases) >= len(cases)
    i = JUNCTION_CASES["middle_1_round"]
    A = arena.shared()
    b = Bufs(A, c, pa, pf, inp=48, h=96, rep=64, off=24)
    flagged = 0
    for row, col, mask, want in cases:
        what = "advice phase %d, fixed phase %d, row %d (instance %d + %d) col %d mask %#x" % (
            pa, pf, row, i, row - int(c.off[i]), col, mask)
        for _, t in b.outputs():
            A.repoison(t)
        try:
            engine.debug_inject(row, col, mask)
            _fused(engine, b, c)
            engine.sync(_stream())
        finally:
            engine.debug_inject(None)
        got = b.report_dict()
        # undo the fault in the written trace: what is left must be the oracle's clean trace
        cell = b.fixed[row:row + 1] if col == 10 else b.advice[col, row:row + 1]
        cell ^= mask - (1 << 32) if mask >> 31 else mask
        _assert_trace(b, c, what + ": written trace ^ mask")
        assert got == want, (what, got, want)
        _assert_guards(A, what)
        flagged += got["first_failure"] != NONE
    assert 3 * flagged >= len(cases), (flagged, len(cases))
    assert torch.equal(c.d_adv, torch.from_numpy(c.adv.view(np.int32)).to(c.d_adv.device))  # the reference stands


# ---------------------------------------------------------------------------------------------
# 4. the split path


def _split_faults(c):
    """Sixteen single-bit faults of the lines24 trace at total_rows = used + 12: (what, col, row,
    bit), col 10 the fixed column. Init region, half-round tile, final region, pad row and fixed
    column; the first (0 rounds), middle (13, 25, 1 rounds) and the last (2 rounds) instance; bits
    0, 15, 16, 31."""
    assert c.name == "lines24" and c.pad == 12 and c.rounds[0] == 0 and c.rounds[6] == 13
    assert c.rounds[10] == 25 and c.rounds[1] == 1 and c.rounds[23] == 2 and c.n == 24
    o = [int(v) for v in c.off]

    def hr(i, h, k):
        assert h < 2 * c.rounds[i] and k < 208
        return o[i] + INIT_ROWS + 208 * h + k

    def fin(i, k):
        assert k < FINAL_ROWS
        return o[i] + INIT_ROWS + ROUND_ROWS * c.rounds[i] + k

    faults = [
        ("init, first", 0, o[0] + 5, 0),
        ("init, middle", 1, o[6] + 100, 15),
        ("init, last", 2, o[23] + 163, 16),
        ("init, middle", 1, o[10] + 40, 31),
        ("half-round, middle", 2, hr(6, 7, 3), 0),
        ("half-round, last", 1, hr(23, 3, 207), 15),
        ("half-round, middle", 0, hr(10, 49, 100), 16),
        ("half-round, middle", 2, hr(1, 0, 0), 31),
        ("final, first", 1, fin(0, 0), 0),
        ("final, middle", 2, fin(6, 33), 15),
        ("final, last row of the batch", 0, fin(23, 63), 16),
        ("pad row", 2, c.used + 5, 31),
        ("fixed, pad row", 10, c.used + 8, 15),
        ("fixed, init, first", 10, o[0], 16),
        ("fixed, half-round, middle", 10, hr(10, 20, 4), 0),
        ("fixed, final, last", 10, fin(23, 62), 31),
    ]
    assert len(faults) == 16 and {f[3] for f in faults} == {0, 15, 16, 31}
    assert max(f[2] for f in faults) < c.total and fin(23, 63) == c.used - 1
    return faults


_SPLIT_VERDICTS = {}


def _split_verdicts(orc, c):
    """The oracle's report on each faulted trace, computed once for the eight phases. Every one
    of the sixteen is flagged: the fast pass must hand each to the exact kernel."""
    if not _SPLIT_VERDICTS:
        adv, fixed = c.adv.copy(), c.fixed.copy()
        out = []
        for what, col, row, bit in _split_faults(c):
            cell = fixed[row:row + 1] if col == 10 else adv[col, row:row + 1]
            cell ^= np.uint32(1 << bit)
            rep = orc.evaluate(adv, fixed, c.off)
            cell ^= np.uint32(1 << bit)
            assert rep["first_failure"] != NONE, (what, col, row, bit)
            out.append(rep)
        _SPLIT_VERDICTS["reports"] = out
    return _SPLIT_VERDICTS["reports"]


@pytest.mark.parametrize("pa", PHASES)
def test_split_path_at_each_phase(engine, orc, pa):
    """b2f_fill_dev then b2f_eval_dev with the advice at each phase and the fixed column 80 bytes
    further round the line: trace, h' and report are the oracle's, the clean trace costs the fast
    pass alone, nothing is written outside the buffers. Then sixteen planted bits, one at a time:
    the report is oracle.evaluate's on the same faulted trace, from the exact kernel."""
    pf = (pa + 80) % 128
    A = arena.shared()
    for name in ("one_0", "one_1", "lines24"):
        c = _case(orc, name, 12)
        what = "%s, advice phase %d, fixed phase %d" % (name, pa, pf)
        A.reset()
        b = Bufs(A, c, pa, pf, inp=(pa + 48) % 128, h=(pa + 32) % 128, rep=(pa + 112) % 128, off=(pa + 8) % 128)
        _fill(engine, b, c)
        _eval(engine, b, c)
        engine.sync(_stream())
        _assert_trace(b, c, what)
        assert b.report_dict() == c.report, what
        assert engine.debug_eval_path() == 0, what
        _assert_guards(A, what)
    verdicts = _split_verdicts(orc, c)
    for (kind, col, row, bit), want in zip(_split_faults(c), verdicts):
        mask32 = -(1 << 31) if bit == 31 else 1 << bit
        cell = b.fixed[row:row + 1] if col == 10 else b.advice[col, row:row + 1]
        A.repoison(b.report)
        cell ^= mask32
        try:
            _eval(engine, b, c)
            engine.sync(_stream())
            got, path = b.report_dict(), engine.debug_eval_path()
        finally:
            cell ^= mask32
        assert got == want, (what, kind, col, row, bit, got, want)
        assert path == 1, (what, kind, col, row, bit)
    _assert_trace(b, c, what + ", faults restored")
    _assert_guards(A, what)


# ---------------------------------------------------------------------------------------------
# 5. the keygen fixed column


@pytest.mark.parametrize("pf", PHASES)
def test_fill_fixed_at_each_phase(engine, orc, pf):
    """b2f_fill_fixed_dev into a column at each phase, the row map 8-byte aligned only: the column
    is oracle.fixed_structure's, zero past the batch, and nothing else is written."""
    import torch

    A = arena.shared()
    for name in ("one_0", "one_1", "lines24"):
        for pad in (0, 12, 1028):
            c = _case(orc, name, pad)
            what = "%s, total_rows = used + %d, fixed phase %d" % (name, pad, pf)
            A.reset()
            off = A.carve(8 * (c.n + 1), (pf + 72) % 128, torch.int64, "offsets")
            fixed = A.carve(4 * c.total, pf, name="fixed")
            off.copy_(c.d_off)
            assert fixed.data_ptr() % 128 == pf and off.data_ptr() % 16 == 8
            engine.fill_fixed_dev(off.data_ptr(), c.n, c.total, fixed.data_ptr(), _stream())
            engine.sync(_stream())
            want = torch.from_numpy(orc.fixed_structure(c.off, c.total).view(np.int32)).to(fixed.device)
            diff = fixed != want
            assert not bool(diff.any()), "%s: differs from the keygen structure at %s" % (what, _rows(diff))
            assert not bool(fixed[c.used:].any()), what
            _assert_guards(A, what)


# ---------------------------------------------------------------------------------------------
# 6. the exports

NROWS = [1, 127, 128, 129, 511, 512, 513, 1025]  # the edges of CELLS_PER_ITER = 128 and XT = 512


def _export_checks(A, out3, want, nrows, what):
    """Rows below nrows of every column are the reference's, the rows from nrows on keep their
    poison, the guards are whole."""
    import torch

    got = out3[:, :nrows]
    ref = torch.from_numpy(np.ascontiguousarray(want).view(np.int64)).to(out3.device)
    if not torch.equal(got, ref):
        diff = (got != ref).any(dim=2)
        col = int(diff.any(dim=1).nonzero()[0])
        assert False, "%s: column %d differs at %s" % (what, col, _rows(diff[col]))
    assert A.is_poison(out3[:, nrows:]), "%s: rows past nrows were written" % what
    _assert_guards(A, what)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_export_fp_at_each_phase(engine, orc, form):
    """b2f_export_fp_dev: the output at each phase, the advice at phase 48 and read from row 1001
    on (4-byte aligned reads), nrows at the edges of the kernel's 128-cell and 512-row steps (the
    BN254 pair-swap meets a last odd pass), out_rows = nrows + 3."""
    import torch

    c = _case(orc, "lines24", 12)
    A = arena.shared()
    adv = A.carve(40 * c.total, 48, name="advice").view(10, c.total)
    adv.copy_(c.d_adv)
    for nrows in NROWS:
        want = orc.export_fp(c.adv, 1001, nrows, form)
        for po in PHASES:
            what = "form %d, nrows %d, output phase %d" % (form, nrows, po)
            A.rewind(1)
            out = A.carve(10 * (nrows + 3) * 32, po, torch.int64, "out")
            engine.export_fp_dev(adv.data_ptr(), c.total, 1001, nrows, form, out.data_ptr(), nrows + 3, _stream())
            engine.sync(_stream())
            _export_checks(A, out.view(10, nrows + 3, 4), want, nrows, what)
    assert torch.equal(adv, c.d_adv)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_export_fixed_fp_at_each_phase(engine, orc, form):
    """b2f_export_fixed_fp_dev: the same row counts from row 101 of a fixed column at phase 80."""
    import ntt_ref as nr
    import quotient_gates_ref as gr
    import torch

    c = _case(orc, "lines24", 12)
    q = c.fixed[101:101 + max(NROWS)]
    assert all(((q >> g) & 1).any() for g in range(16)) and (q >> 16).any()
    full = np.stack([nr.pack(col, form) for col in gr.unpack_fixed(q)])
    A = arena.shared()
    fixed = A.carve(4 * c.total, 80, name="fixed")
    fixed.copy_(c.d_fixed)
    for nrows in NROWS:
        for po in PHASES:
            what = "form %d, nrows %d, output phase %d" % (form, nrows, po)
            A.rewind(1)
            out = A.carve(17 * (nrows + 3) * 32, po, torch.int64, "out")
            engine.export_fixed_fp_dev(fixed.data_ptr(), c.total, 101, nrows, form, out.data_ptr(), nrows + 3,
                                       _stream())
            engine.sync(_stream())
            _export_checks(A, out.view(17, nrows + 3, 4), full[:, :nrows], nrows, what)
    assert torch.equal(fixed, c.d_fixed)


@pytest.mark.parametrize("form", [1, 3])
def test_spread_table_at_16_byte_phases(engine, form):
    """b2f_spread_table_dev at phases 16 and 112, out_rows = usable_rows + 1: the three columns
    are (tag, dense, spread) of every x < 2^16 and the row-0 default beyond, row usable_rows of
    each column keeps its poison."""
    import lookup as lk
    import ntt_ref as nr
    import torch

    usable = (1 << 16) + 300
    cols = ([lk.tag(x) for x in range(1 << 16)], list(range(1 << 16)), [lk.spread(x) for x in range(1 << 16)])
    want = np.stack([nr.pack(col + [0] * 300, form) for col in cols])
    A = arena.shared()
    for po in (16, 112):
        A.reset()
        out = A.carve(3 * (usable + 1) * 32, po, torch.int64, "out")
        engine.spread_table_dev(usable, form, out.data_ptr(), usable + 1, _stream())
        engine.sync(_stream())
        _export_checks(A, out.view(3, usable + 1, 4), want, usable, "form %d, output phase %d" % (form, po))


# ---------------------------------------------------------------------------------------------
# 7. refusals: 8 bytes past a 16-byte boundary


def _refused(engine, call, A, b, what):
    """`call` raises B2F_ERR_ARG and writes nothing: the output buffers and everything outside the
    carves are still poison."""
    import b2f

    with pytest.raises(b2f.B2FError) as e:
        call()
    assert e.value.code == ERR_ARG, (what, e.value)
    engine.sync(_stream())
    for name, t in b:
        assert A.is_poison(t), "%s: refused, yet %s was written" % (what, name)
    _assert_guards(A, what)


@pytest.mark.parametrize("call", ["fill_dev", "fill_eval_dev"])
def test_fill_refuses_8_byte_alignment(engine, orc, call):
    """b2f_fill_dev and b2f_fill_eval_dev: d_in, d_advice and d_fixed each moved to 8 bytes past a
    16-byte boundary, one at a time, are B2F_ERR_ARG with nothing written; the good call that
    follows on the same context is right."""
    c = _case(orc, "one_1", 12)
    A = arena.shared()
    b = Bufs(A, c, 16, 80, inp=48, h=96, rep=64, off=24)

    def run(d_in=0, d_adv=0, d_fix=0):
        args = (b.inputs.data_ptr() + d_in, c.n, b.offsets.data_ptr(), c.total, b.advice.data_ptr() + d_adv,
                b.fixed.data_ptr() + d_fix, b.h_out.data_ptr())
        if call == "fill_dev":
            engine.fill_dev(*args, _stream())
        else:
            engine.fill_eval_dev(*args, b.report.data_ptr(), _stream())

    for kw in ({"d_in": 8}, {"d_adv": 8}, {"d_fix": 8}):
        _refused(engine, lambda: run(**kw), A, b.outputs(), "%s %s" % (call, kw))
    run()
    engine.sync(_stream())
    _assert_trace(b, c, call + " after the refusals")
    if call == "fill_eval_dev":
        assert b.report_dict() == c.report
    else:
        assert A.is_poison(b.report)
    _assert_guards(A, call)


def test_eval_refuses_8_byte_alignment(engine, orc):
    """b2f_eval_dev: d_advice and d_fixed at 8 bytes past a 16-byte boundary."""
    c = _case(orc, "one_1", 12)
    A = arena.shared()
    b = Bufs(A, c, 112, 32, rep=16, off=8)
    b.advice.copy_(c.d_adv)
    b.fixed.copy_(c.d_fixed)

    def run(d_adv=0, d_fix=0):
        engine.eval_dev(b.advice.data_ptr() + d_adv, b.fixed.data_ptr() + d_fix, b.offsets.data_ptr(), c.n,
                        c.total, b.report.data_ptr(), _stream())

    for kw in ({"d_adv": 8}, {"d_fix": 8}):
        _refused(engine, lambda: run(**kw), A, (("report", b.report),), "eval_dev %s" % kw)
    run()
    engine.sync(_stream())
    assert b.report_dict() == c.report
    _assert_trace(b, c, "eval_dev after the refusals", h=False)  # the call only reads the trace
    _assert_guards(A, "eval_dev")


def test_fill_fixed_refuses_8_byte_alignment(engine, orc):
    """b2f_fill_fixed_dev: d_fixed at 8 bytes past a 16-byte boundary."""
    import torch

    c = _case(orc, "one_1", 12)
    A = arena.shared()
    off = A.carve(8 * (c.n + 1), 8, torch.int64, "offsets")
    fixed = A.carve(4 * c.total + 16, 48, name="fixed")
    off.copy_(c.d_off)
    _refused(engine, lambda: engine.fill_fixed_dev(off.data_ptr(), c.n, c.total, fixed.data_ptr() + 8, _stream()),
             A, (("fixed", fixed),), "fill_fixed_dev")
    engine.fill_fixed_dev(off.data_ptr(), c.n, c.total, fixed.data_ptr(), _stream())
    engine.sync(_stream())
    assert torch.equal(fixed[:c.total], c.d_fixed) and A.is_poison(fixed[c.total:])
    _assert_guards(A, "fill_fixed_dev")


@pytest.mark.parametrize("call", ["export_fp_dev", "export_fixed_fp_dev"])
def test_exports_refuse_8_byte_alignment(engine, orc, call):
    """b2f_export_fp_dev and b2f_export_fixed_fp_dev: d_out at 8 bytes past a 16-byte boundary."""
    import ntt_ref as nr
    import quotient_gates_ref as gr
    import torch

    c = _case(orc, "one_1", 12)
    form, nrows, rb = 3, 129, 101
    A = arena.shared()
    if call == "export_fp_dev":
        ncols, src, ref = 10, A.carve(40 * c.total, 48, name="advice"), c.d_adv
        want = orc.export_fp(c.adv, rb, nrows, form)
    else:
        ncols, src, ref = 17, A.carve(4 * c.total, 80, name="fixed"), c.d_fixed
        want = np.stack([nr.pack(col, form) for col in gr.unpack_fixed(c.fixed[rb:rb + nrows])])
    src.copy_(ref.reshape(-1))
    out = A.carve(ncols * (nrows + 3) * 32 + 16, 112, torch.int64, "out")

    def run(d_out=0):
        getattr(engine, call)(src.data_ptr(), c.total, rb, nrows, form, out.data_ptr() + d_out, nrows + 3, _stream())

    _refused(engine, lambda: run(8), A, (("out", out),), call)
    run()
    engine.sync(_stream())
    _export_checks(A, out[:ncols * (nrows + 3) * 4].view(ncols, nrows + 3, 4), want, nrows, call + " after the refusal")
    assert A.is_poison(out[ncols * (nrows + 3) * 4:])
