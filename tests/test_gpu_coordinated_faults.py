"""Constraint-consistent multi-cell faults (tests/coordinated_faults.py, pinned on the CPU by
tests/test_coordinated_faults_ref.py) through the two checkers that decide a verdict on a trace in
memory: the product eval (the fast clean-check pass, eval_hr_kernel / eval_edge_kernel, handing
over to the exact kernel) and the exact 1,024-row-tile kernel alone.

The single-bit sweep (tests/test_gpu_cell_sweep.py) breaks several constraint families with every
fault; here each class leaves all families but one intact, so a family of the fast pass that checked
nothing would let its class through on path 0 with a clean report: L (lookups hold: gates and
copies), C (lookups and copies hold: gates, gate 14 and the message copy's 14-cell classes among
them), S (every gate zero over Z: copies), W (the XOR sum zero mod 2^32 only: the exact kernel must
count the gate), T (the XOR sum kept: tags and recompositions), R (everything but a range holds mod
2^32 down to the digest: the tag and a_6 range terms alone). 7,227 faults on batch A and 3,014
on batch B's windows and message limbs per checker, 20,482 in the file. One test per (checker, class);
the device traces are filled once per module and stay resident; a fault is one indexed write over
a flat view of the advice tensor, one run, the 176-byte report read back, one indexed write back.

  product  b2f_eval_dev: the report is the oracle's as a whole; when the oracle rejects, the fast
           pass handed over to the exact kernel (path 1); when it accepts (the zero rows of class L)
           the report is the clean one (a hand-over is counted and printed, no failure).
  exact    the diagnostics build with B2F_DIAG_EVAL=23 (the exact kernel alone, path 2): the report
           is the oracle's for every fault: W's gate counter, S's untouched gate counters.

After each class the trace is bit for bit the clean one and clean to the checker on its path. Each
test asserts how many faults it compared and how many the oracle rejected, the numbers the
reference test pins. Needs an MI355X (`-m gpu`).

Measured durations (MI355X, one `--durations=0` run of this module, 12 tests in 6.0 s): product L
0.77 s, C 0.67 s, S 0.86 s, W 0.23 s, T 0.04 s, R 0.03 s (its first look at a fault pays the
oracle's CPU evaluation; about 190 us a fault on batch A and 420 us on batch B in all); exact L
0.25 s, C 0.21 s, S 0.27 s, W 0.07 s, T and R 0.01 s (about 72 us a fault on batch A, 95 us on batch
B); the module's setup 2.06 s, of which the session's engine is a part when the module runs alone.
In that run no accepted fault (the 8 zero rows of class L) was handed to the exact kernel.
"""
import os
import time

import pytest

import cell_sweep as cs
import coordinated_faults as cf

pytestmark = pytest.mark.gpu

MAX_SHOWN = 8  # mismatches listed before a test gives up


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Resident:
    """A batch on the device with a clean copy of its trace, and per class the faults as three
    device vectors (flat cell index, new value, clean value) cut by `span`."""

    def __init__(self, engine, name):
        import numpy as np
        import torch

        import b2f

        self.name = name
        self.host = hb = cs.batch(name)
        self.faults = fs = cf.faults(name)
        self.dev = db = b2f.DeviceBatch(hb.inputs, total_rows=hb.total)
        db.advice.fill_(-1)
        db.fixed.fill_(-1)
        db.fill(engine)
        engine.sync(_stream())
        dev = db.advice.device
        self.adv = torch.from_numpy(hb.adv.view(np.int32)).to(dev)
        self.fixed = torch.from_numpy(hb.fixed.view(np.int32)).to(dev)
        assert torch.equal(db.advice, self.adv) and torch.equal(db.fixed, self.fixed), \
            "the device fill is not the oracle's trace"
        assert db.advice.is_contiguous()
        self.flat = db.advice.view(-1)
        self.idx, self.new, self.old, self.span = {}, {}, {}, {}
        for cls in cf.CLASSES:
            idx, new, span = [], [], []
            for f in fs.by_class[cls]:
                span.append((len(idx), len(idx) + len(f.writes)))
                for c, r, v in f.writes:
                    assert 0 <= r < hb.total
                    idx.append(c * hb.total + r)
                    new.append(v)
            self.idx[cls] = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
            self.new[cls] = torch.from_numpy(np.asarray(new, dtype=np.uint32).view(np.int32)).to(dev)
            self.old[cls] = self.adv.view(-1)[self.idx[cls]].clone()
            self.span[cls] = span

    def write(self, cls, k, values):
        s, e = self.span[cls][k]
        self.flat[self.idx[cls][s:e]] = values[cls][s:e]

    def restore(self):
        self.dev.advice.copy_(self.adv)
        self.dev.fixed.copy_(self.fixed)

    def is_clean(self):
        import torch

        return torch.equal(self.dev.advice, self.adv) and torch.equal(self.dev.fixed, self.fixed)


@pytest.fixture(scope="module")
def resident(engine, orc):
    return {name: Resident(engine, name) for name in ("A", "B")}


def _run(eng, res, cls, k):
    db = res.dev
    res.write(cls, k, res.new)
    try:
        db.evaluate(eng)
        path = eng.debug_eval_path()
        rep = db.report_dict()
    finally:
        res.write(cls, k, res.old)
    return rep, path


def _product(rep, path, want, clean, stats):
    if rep != want:
        return "report %r != oracle %r (path %d)" % (rep, want, path)
    if cf.rejected(want):
        if path != 1:
            return "the fast pass let it through (path %d)" % path
    else:
        if rep != clean or path not in (0, 1):
            return "an accepted fault changed the report (path %d): %r" % (path, rep)
        stats["accepted faults handed over"] += path
    return None


def _exact(rep, path, want, clean, stats):
    if path != 2:
        return "path %d: the exact kernel did not run alone" % path
    if rep != want:
        return "report %r != oracle %r" % (rep, want)
    return None


@pytest.mark.parametrize("cls", cf.CLASSES)
@pytest.mark.parametrize("checker", ["product", "exact"])
def test_coordinated_faults(engine, diag_engine, resident, checker, cls):
    judge = {"product": _product, "exact": _exact}[checker]
    eng = diag_engine if checker == "exact" else engine
    assert "B2F_DIAG_EVAL" not in os.environ
    try:
        if checker == "exact":
            os.environ["B2F_DIAG_EVAL"] = "23"
        for name in ("A", "B"):
            res = resident[name]
            hb, fs = res.host, res.faults
            res.restore()
            stats = {"accepted faults handed over": 0}
            cases = rejected = 0
            bad = []
            t0 = time.perf_counter()
            for k, f in enumerate(fs.by_class[cls]):
                want = cf.verdict(name, f)
                rep, path = _run(eng, res, cls, k)
                cases += 1
                rejected += cf.rejected(want)
                why = judge(rep, path, want, hb.clean, stats)
                if why is not None:
                    bad.append("batch %s %r: %s" % (name, f, why))
                    if len(bad) >= MAX_SHOWN:
                        break
            dt = time.perf_counter() - t0
            print("%s, class %s, batch %s: %d faults compared (%d rejected by the oracle%s), %.0f us each"
                  % (checker, cls, name, cases, rejected,
                     ", %d accepted faults handed to the exact kernel" % stats["accepted faults handed over"]
                     if checker == "product" else "", 1e6 * dt / max(cases, 1)))
            assert not bad, "\n".join(bad)
            assert (cases, rejected) == (cf.COUNTS[name][cls][0], cf.COUNTS[name][cls][3])
            # the batch after the class: bit for bit the clean one, and clean to the checker
            assert res.is_clean(), "the restored trace is not the clean one"
            res.dev.evaluate(eng)
            path = eng.debug_eval_path()
            assert res.dev.report_dict() == hb.clean
            assert path == (0 if checker == "product" else 2), path
    finally:
        os.environ.pop("B2F_DIAG_EVAL", None)
        for res in resident.values():
            res.restore()
