"""The trace kernels on structured inputs: the batch of tests/structured_inputs.py (2,002 instances,
whole-word extremes that uniform draws never reach: ADD results of exactly 0 with carry 1 and 2,
all-ones words, XOR outputs of 0 and all ones, the rot-63 split at zb = 1 / 0x7fff, the rot-24
pieces at 0xff) through the fill, the product eval (the fast clean-check pass must call these
values clean itself: path 0), the exact kernel alone, the fused pass and its advice-only repeat
call; single-bit faults aimed at the extreme blocks through the three checkers; the hasher on
all-zero and all-0xff messages and keys; and the lookup columns of a circuit whose input column
holds a few dozen distinct values, tens of thousands of times each.

The reference is the CPU oracle's trace and report of the same batch, built once
(structured_inputs.reference(); pinned by tests/test_structured_inputs_ref.py, which also shows
that every census class is reached), and f_ref for h'. No test compares the GPU with itself.

Needs an MI355X (`-m gpu`).

Measured durations (MI355X, one `--durations=0` run of the whole `-m gpu` suite, 568 tests in
166 s): the module's setup (the oracle's 5,765,040-row trace, its census, f_ref on 2,002 instances,
the upload) 0.23 s, or 2.5 s when this file runs alone and is the first to touch the GPU; the 128
faults 0.06 s through the product eval, 0.07 s through the exact kernel, 0.12 s through the fused
pass (0.45 to 0.95 ms a fault, the oracle's windowed evaluation included); a lookup test 0.38 s
(most of it oracle/lookup.py on 2^16 rows); the fill, eval, fused and hasher tests under 0.2 s
each; the 17 tests together under 5 s.
"""
import hashlib
import os

import numpy as np
import pytest

import structured_inputs as si
from cell_sweep import dev_flip32
from verdict_util import NONE, dev_flip

pytestmark = pytest.mark.gpu

POISON = -0x21524111  # 0xdeadbeef as int32
RESIDENT = 1  # B2F_FIXED_RESIDENT
CHECKERS = ("product", "exact", "fused")
MAX_SHOWN = 12


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Resident:
    """The structured batch on the device, with the oracle's trace and the reference h' beside it."""

    def __init__(self, ref):
        import torch

        import b2f

        self.ref = ref
        self.dev = db = b2f.DeviceBatch(ref.inputs, total_rows=ref.total)
        dev = db.advice.device
        self.adv = torch.from_numpy(ref.adv.view(np.int32)).to(dev)
        self.fixed = torch.from_numpy(ref.fixed.view(np.int32)).to(dev)
        assert np.array_equal(ref.h_out, ref.h_ref), "the oracle's h' is not f_ref's"
        self.h_out = torch.from_numpy(ref.h_ref.view(np.int64)).to(dev)

    def poison(self, fixed=True):
        db = self.dev
        db.advice.fill_(POISON)
        if fixed:
            db.fixed.fill_(POISON)
        db.h_out.fill_(-1)
        db.report.fill_(-1)

    def restore(self):
        """The device trace := the oracle's."""
        self.dev.advice.copy_(self.adv)
        self.dev.fixed.copy_(self.fixed)
        self.dev.h_out.copy_(self.h_out)

    def is_clean(self):
        import torch

        db = self.dev
        return (torch.equal(db.advice, self.adv) and torch.equal(db.fixed, self.fixed)
                and torch.equal(db.h_out, self.h_out))

    def assert_trace(self, fixed=True):
        """Every column bit-equal to the oracle's, the first differing rows named; h' equal to the
        oracle's and f_ref's (one array: checked equal above); the rows past the batch zero."""
        db, ref = self.dev, self.ref
        diffs = []
        for c in range(10):
            bad = (db.advice[c] != self.adv[c]).nonzero().reshape(-1)
            if len(bad):
                diffs.append("a_%d differs at %d rows, first %s" % (c, len(bad), bad[:8].tolist()))
        if fixed:
            bad = (db.fixed != self.fixed).nonzero().reshape(-1)
            if len(bad):
                diffs.append("fixed differs at %d rows, first %s" % (len(bad), bad[:8].tolist()))
        bad = (db.h_out != self.h_out).any(dim=1).nonzero().reshape(-1)
        if len(bad):
            diffs.append("h' differs at %d instances, first %s" % (len(bad), bad[:8].tolist()))
        assert not diffs, "\n".join(diffs)
        assert not db.advice[:, ref.used:].any() and (not fixed or not db.fixed[ref.used:].any())
        assert ref.total - ref.used == si.PAD_ROWS


@pytest.fixture(scope="module")
def ref(orc):
    r = si.reference()
    assert r.clean["first_failure"] == NONE and r.clean["rows_checked"] == r.total
    assert all(len(r.census[c]) for c in si.CLASSES)
    return r


@pytest.fixture(scope="module")
def res(engine, ref):
    return Resident(ref)


def test_fill_equals_oracle(engine, res, ref):
    db = res.dev
    res.poison()
    db.fill(engine)
    engine.sync(_stream())
    res.assert_trace()
    assert np.array_equal(db.offsets.cpu().numpy().view(np.uint64), ref.off)
    assert np.array_equal(db.host_h_out(), ref.h_ref)


def test_product_eval_calls_the_filled_trace_clean(engine, res, ref):
    """The report is the oracle's, and the fast clean-check pass found it itself: a false flag
    there would show as path 1 with the same clean report."""
    db = res.dev
    res.poison()
    db.fill(engine)
    db.evaluate(engine)
    path = engine.debug_eval_path()
    assert db.report_dict() == ref.clean
    assert path == 0, "the fast pass flagged a clean trace (path %d)" % path
    res.assert_trace()


def test_exact_kernel_alone(engine, diag_engine, res, ref):
    db = res.dev
    res.poison()
    db.fill(engine)
    assert "B2F_DIAG_EVAL" not in os.environ
    try:
        os.environ["B2F_DIAG_EVAL"] = "23"
        db.evaluate(diag_engine)
        path = diag_engine.debug_eval_path()
        rep = db.report_dict()
    finally:
        os.environ.pop("B2F_DIAG_EVAL", None)
    assert rep == ref.clean
    assert path == 2, path
    res.assert_trace()


def _fused_call(eng, db, flags):
    eng.fill_eval_dev(db.inputs.data_ptr(), db.n, db.offsets.data_ptr(), db.total_rows,
                      db.advice.data_ptr(), db.fixed.data_ptr(), db.h_out.data_ptr(),
                      db.report.data_ptr(), _stream(), flags=flags)


def test_fused_pass_and_resident_repeat(engine, res, ref):
    db = res.dev
    res.poison()
    db.fill_evaluate(engine, fixed_resident=False)
    assert engine.debug_fused_path() == 0
    engine.sync(_stream())
    assert db.report_dict() == ref.clean
    res.assert_trace()
    # the repeat call: advice-only, over a sentinel in `fixed` that must survive it
    res.poison()
    _fused_call(engine, db, RESIDENT)
    assert engine.debug_fused_path() == 1
    engine.sync(_stream())
    left = (db.fixed != POISON).nonzero().reshape(-1).tolist()
    assert left == [], "fixed written at rows %s" % left[:10]
    assert db.report_dict() == ref.clean
    res.assert_trace(fixed=False)
    db.invalidate_fixed()
    res.restore()


def _product(engine, res, col, row, mask, want):
    db = res.dev
    dev_flip(db, col, row, mask)
    try:
        db.evaluate(engine)
        path = engine.debug_eval_path()
        rep = db.report_dict()
    finally:
        dev_flip(db, col, row, mask)
    if rep != want:
        return "report %r != oracle %r (path %d)" % (rep, want, path)
    if path != 1:
        return "the fault was not handed to the exact kernel (path %d)" % path
    return None


def _exact(diag_engine, res, col, row, mask, want):
    db = res.dev
    dev_flip(db, col, row, mask)
    try:
        db.evaluate(diag_engine)
        path = diag_engine.debug_eval_path()
        rep = db.report_dict()
    finally:
        dev_flip(db, col, row, mask)
    if path != 2:
        return "path %d: the exact kernel did not run alone" % path
    if rep != want:
        return "report %r != oracle %r" % (rep, want)
    return None


def _fused(engine, res, col, row, mask, want):
    db = res.dev
    res.poison()
    try:
        engine.debug_inject(row, col, mask)
        db.fill_evaluate(engine)
        engine.sync(_stream())
    finally:
        engine.debug_inject(None)
    if engine.debug_fused_path() != 0:
        return "the advice-only kernel ran under the inject hook"
    rep = db.report_dict()
    dev_flip32(db, col, row, mask)  # the written trace with that one cell XORed back
    if not res.is_clean():
        return "the written trace or h' differs from the oracle's beyond the injected cell"
    if rep != want:
        return "report %r != oracle %r" % (rep, want)
    return None


@pytest.mark.parametrize("checker", CHECKERS)
def test_faults_in_the_extreme_blocks(engine, diag_engine, res, ref, checker):
    """Up to four blocks of every census class; in each, bit 0 of a result limb (a_1) and of an
    operand limb (a_3), and in the ADD blocks bit 0 of the carry (a_9; bit 1 too where it is 2).
    Every fault is rejected by the oracle, and the checker's report is the oracle's."""
    import time

    run = {"product": _product, "exact": _exact, "fused": _fused}[checker]
    eng = diag_engine if checker == "exact" else engine
    cases = si.faults(ref.census, ref.adv)
    assert {c[0] for c in cases} == set(si.CLASSES)
    assert any(c[1] == 9 and c[3] == 2 for c in cases), "no carry of 2 among the faults"
    assert "B2F_DIAG_EVAL" not in os.environ
    res.restore()
    bad = []
    t0 = time.perf_counter()
    try:
        if checker == "exact":
            os.environ["B2F_DIAG_EVAL"] = "23"
        for cls, col, row, mask in cases:
            want = ref.verdict(col, row, mask)
            assert want["first_failure"] != NONE, ("the oracle accepts", cls, col, row, mask)
            why = run(eng, res, col, row, mask, want)
            if why is not None:
                bad.append((cls, col, row, hex(mask), why))
                if len(bad) >= MAX_SHOWN:
                    break
    finally:
        os.environ.pop("B2F_DIAG_EVAL", None)
        engine.debug_inject(None)
        res.dev.invalidate_fixed()
        res.restore()
    print("%s: %d faults over %d classes, %.0f us each"
          % (checker, len(cases), len(si.CLASSES), 1e6 * (time.perf_counter() - t0) / len(cases)))
    assert not bad, "\n".join(str(b) for b in bad)
    assert res.is_clean()


HASH_LENGTHS = (0, 1, 127, 128, 129, 255, 256, 1024)


@pytest.mark.parametrize("path", ["split", "fused"])
@pytest.mark.parametrize("key", [b"", bytes(64), b"\xff" * 64, b"\xff"], ids=["nokey", "key00x64", "keyffx64", "keyff"])
def test_hasher_on_constant_messages(engine, path, key):
    from b2f import hasher

    msgs = [bytes([b]) * n for b in (0x00, 0xff) for n in HASH_LENGTHS]
    out = hasher.blake2b_batch(engine, msgs, 64, key, path=path)
    assert out.verified, [r for r in out.reports if r["first_failure"] != NONE][:1]
    assert len(out.reports) == 8 + (1 if key else 0)
    for m, d in zip(msgs, out.digests):
        assert d == hashlib.blake2b(m, key=key).digest(), (len(m), m[:1])


def _limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)


@pytest.fixture(scope="module")
def extreme_circuit(orc):
    """One all-extreme 0-round instance (h = m = t = all ones, f = 1) repeated until the trace
    passes 2^16 + 2^10 rows, and the oracle's lookup cells of its first 2^16 rows."""
    x = si.batch()[:1].copy()
    assert si.special_positions()[0] == "all_extreme" and int(x["h"][0][0]) == si.M64 and int(x["f"][0]) == 1
    x["rounds"] = 0
    reps = -(-((1 << 16) + (1 << 10)) // 228)
    x = np.repeat(x, reps)
    adv, _, _, off = orc.fill(x)
    assert (1 << 16) + (1 << 10) <= int(off[-1]) < (1 << 16) + (1 << 10) + 228
    return x, adv[:3, :1 << 16].copy()


@pytest.mark.parametrize("form", [1, 3])
def test_lookup_columns_of_a_few_values(engine, extreme_circuit, form):
    """usable_rows = 2^16, the smallest the call accepts: A, S, A', S' and z against
    oracle/lookup.py on the oracle's cells."""
    import lookup as lk
    import torch

    import b2f

    x, a = extreme_circuit
    usable = 1 << 16
    vals, mult = np.unique(a[1], return_counts=True)
    assert len(vals) < 100 and int(mult.max()) > 20000, (len(vals), int(mult.max()))
    p = lk.P_BN254 if form & 2 else lk.P
    r = np.random.default_rng(90 + form)
    theta, beta, gamma = [int.from_bytes(r.bytes(32), "little") % p for _ in range(3)]
    db = b2f.DeviceBatch(x)
    db.fill(engine)
    out, bad = db.lookup_columns(engine, [0], usable, theta, beta, gamma, form=form)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    assert (bad.cpu().numpy().view(np.uint64) == np.uint64(NONE)).all()
    assert np.array_equal(db.advice[:3, :usable].cpu().numpy().view(np.uint32), a)
    got = out.cpu().numpy().view(np.uint64)
    want = lk.columns(a[0], a[1], a[2], usable, theta, beta, gamma, p)
    assert want[4][-1] == 1
    R = 1 << 256
    diffs = []
    for j, name in enumerate(["A", "S", "A'", "S'", "z"]):
        n = usable + 1 if j == 4 else usable
        w = _limbs([v * R % p for v in want[j]])
        ne = np.nonzero((got[0, j, :n] != w).any(axis=1))[0]
        if len(ne):
            diffs.append("column %s differs first at row %d (%d rows differ)" % (name, int(ne[0]), len(ne)))
    assert not diffs, "; ".join(diffs)
