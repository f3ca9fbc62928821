"""Single-bit faults in every trace cell through the three checkers that decide a verdict: the
product eval (the fast clean-check pass, eval_hr_kernel / eval_edge_kernel, handing over to the
exact kernel), the exact 1,024-row-tile kernel alone, and the fused pass's on-CU checks.

The batches, masks, the derived set of constrained cells and the oracle's report per fault are
tests/cell_sweep.py's (pinned on the CPU by tests/test_cell_sweep_ref.py): all 28,424 cells of
batch A (the cells of its 2-round instance with bits 0, 15, 16 and 31 each) and the windows of
batch B, 6,452 faults per column, 70,972 per checker, 212,916 in the file. One test per (checker,
column); the device traces are filled once per module and stay resident; a fault is one cell
flipped on the device (or injected as the fused pass assigns it), one run, the 176-byte report
read back, the cell restored.

  product  b2f_eval_dev: the report is the oracle's as a whole; a fault in a constrained cell was
           handed to the exact kernel (path 1); a fault in a free cell leaves the clean report (the
           fast pass may still hand over: counted and printed, no failure).
  exact    the diagnostics build with B2F_DIAG_EVAL=23 (the clocked full kernel: diagnostic modes
           run the exact kernel alone, path 2): the report is the oracle's for every fault, the
           free cells included, which the product path never shows to this kernel.
  fused    b2f_debug_inject + b2f_fill_eval_dev over poisoned buffers: the report is the oracle's,
           the written trace is the clean one but for that cell (compared on the device), h' is
           the clean h', the full kernel ran.

Each test asserts how many faults it compared and how many of them were in constrained cells.
Needs an MI355X (`-m gpu`).

Measured durations (MI355X, one `--durations=0` run of the whole `-m gpu` suite, 491 tests in
150 s; its slowest test, test_gpu_bench.py::test_bench_rccl_code_path_one_rank, took 6.37 s), per
test of 6,452 faults: product 1.18-1.56 s (its first look at a fault pays the oracle's CPU
evaluation, about 130 us on batch A and 300 us on batch B's window; the GPU side is about 70 us),
exact 0.46-0.48 s (about 70 us a fault), fused 1.79-1.92 s (about 265 us a fault on batch A, 390
us on batch B), the module's setup 0.41 s; the 33 tests together 41 s. In that run no free cell was
handed to the exact kernel by the product's fast pass.
"""
import os
import time

import pytest

import cell_sweep as cs

pytestmark = pytest.mark.gpu

CHECKERS = ("product", "exact", "fused")
MAX_SHOWN = 12  # mismatches listed before a test gives up


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Resident:
    """A sweep batch on the device, with clean copies of the trace and h'."""

    def __init__(self, engine, name):
        import numpy as np
        import torch

        import b2f

        self.host = hb = cs.batch(name)
        self.dev = db = b2f.DeviceBatch(hb.inputs, total_rows=hb.total)
        db.advice.fill_(-1)
        db.fixed.fill_(-1)
        db.fill(engine)
        engine.sync(_stream())
        dev = db.advice.device
        self.adv = torch.from_numpy(hb.adv.view(np.int32)).to(dev)
        self.fixed = torch.from_numpy(hb.fixed.view(np.int32)).to(dev)
        self.h_out = db.h_out.clone()
        assert torch.equal(db.advice, self.adv) and torch.equal(db.fixed, self.fixed), \
            "the device fill is not the oracle's trace"
        assert np.array_equal(db.host_h_out(), hb.h_out)

    def restore(self):
        self.dev.advice.copy_(self.adv)
        self.dev.fixed.copy_(self.fixed)
        self.dev.h_out.copy_(self.h_out)

    def is_clean(self):
        import torch

        db = self.dev
        return (torch.equal(db.advice, self.adv) and torch.equal(db.fixed, self.fixed)
                and torch.equal(db.h_out, self.h_out))


@pytest.fixture(scope="module")
def resident(engine, orc):
    return {name: Resident(engine, name) for name in ("A", "B")}


def _product(engine, res, col, row, mask, want, con, stats):
    db = res.dev
    cs.dev_flip32(db, col, row, mask)
    try:
        db.evaluate(engine)
        path = engine.debug_eval_path()
        rep = db.report_dict()
    finally:
        cs.dev_flip32(db, col, row, mask)
    if rep != want:
        return "report %r != oracle %r (path %d)" % (rep, want, path)
    if con and path != 1:
        return "a fault in a constrained cell was not handed to the exact kernel (path %d)" % path
    if not con:
        if rep != res.host.clean or path not in (0, 1):
            return "a fault in a free cell changed the report (path %d): %r" % (path, rep)
        stats["free cells handed over"] += path
    return None


def _exact(diag_engine, res, col, row, mask, want, con, stats):
    db = res.dev
    cs.dev_flip32(db, col, row, mask)
    try:
        db.evaluate(diag_engine)
        path = diag_engine.debug_eval_path()
        rep = db.report_dict()
    finally:
        cs.dev_flip32(db, col, row, mask)
    if path != 2:
        return "path %d: the exact kernel did not run alone" % path
    if rep != want:
        return "report %r != oracle %r" % (rep, want)
    return None


def _fused(engine, res, col, row, mask, want, con, stats):
    db = res.dev
    db.advice.fill_(-1)
    db.fixed.fill_(-1)
    db.h_out.fill_(-1)
    try:
        engine.debug_inject(row, col, mask)
        db.fill_evaluate(engine)
        engine.sync(_stream())
    finally:
        engine.debug_inject(None)
    if engine.debug_fused_path() != 0:
        return "the advice-only kernel ran under the inject hook"
    rep = db.report_dict()
    cs.dev_flip32(db, col, row, mask)  # the written trace with that one cell XORed back
    if not res.is_clean():
        return "the written trace or h' differs from the clean one beyond the injected cell"
    if rep != want:
        return "report %r != oracle %r" % (rep, want)
    return None


def _after(checker, engine, diag_engine, res):
    """The batch after its sweep: bit for bit the clean one, and clean to the checker."""
    db, clean = res.dev, res.host.clean
    if checker == "fused":
        db.advice.fill_(-1)
        db.fixed.fill_(-1)
        db.h_out.fill_(-1)
        db.fill_evaluate(engine)
        engine.sync(_stream())
        assert db.report_dict() == clean, "the fused call without the hook is not clean"
        assert res.is_clean()
        return
    assert res.is_clean(), "the restored trace is not the clean one"
    eng = engine if checker == "product" else diag_engine
    db.evaluate(eng)
    path = eng.debug_eval_path()
    assert db.report_dict() == clean
    assert path == (0 if checker == "product" else 2), path


@pytest.mark.parametrize("col", range(cs.NCOLS))
@pytest.mark.parametrize("checker", CHECKERS)
def test_every_cell_fault(engine, diag_engine, resident, checker, col):
    run = {"product": _product, "exact": _exact, "fused": _fused}[checker]
    eng = diag_engine if checker == "exact" else engine
    assert "B2F_DIAG_EVAL" not in os.environ
    try:
        if checker == "exact":
            os.environ["B2F_DIAG_EVAL"] = "23"
        for name in ("A", "B"):
            res = resident[name]
            hb = res.host
            res.restore()
            stats = {"free cells handed over": 0}
            cases = constrained = 0
            bad = []
            t0 = time.perf_counter()
            for row, mask in hb.cases(col):
                con = bool(hb.constrained[col, row])
                want = cs.oracle_verdict(name, col, row, mask)
                assert cs.rejected(want) == con, (name, col, row, mask)
                why = run(eng, res, col, row, mask, want, con, stats)
                cases += 1
                constrained += con
                if why is not None:
                    bad.append((name, col, row, hex(mask), "constrained" if con else "free", why))
                    if len(bad) >= MAX_SHOWN:
                        break
            dt = time.perf_counter() - t0
            print("%s, column %d, batch %s: %d faults compared (%d in constrained cells%s), %.0f us each"
                  % (checker, col, name, cases, constrained,
                     ", %d free cells handed to the exact kernel" % stats["free cells handed over"]
                     if checker == "product" else "", 1e6 * dt / max(cases, 1)))
            assert not bad, "\n".join(str(b) for b in bad)
            assert cases == hb.n_cases() == len(hb.rows) + 3 * (hb.four[1] - hb.four[0])
            assert constrained == hb.n_constrained_cases(col)
            _after(checker, engine, diag_engine, res)
    finally:
        os.environ.pop("B2F_DIAG_EVAL", None)
        engine.debug_inject(None)
        for res in resident.values():
            res.restore()
