"""The prover calls on a caller-owned, non-blocking stream, queued behind in-flight work.

include/b2f.h promises that every `*_dev` call is stream-ordered on the caller's stream. The rest
of the GPU suite runs on the null stream with a host sync after nearly every call, which hides the
mistakes a caller's stream exposes: a clear that is not ordered against the next call's kernels,
fork / join events that wait for the wrong thing, pinned staging rewritten before its upload ran,
a cached table read before its fill. Everything here runs inside `with torch.cuda.stream(side)`
(`side = torch.cuda.Stream()`: torch's pool streams are non-blocking), expected values come from
the big-integer references, and results are read back only after the last call of a sequence.

Scenarios 1 to 5 run twice on one fresh engine:
  cold    the first calls grow scratch and may block the host;
  queued  same shapes, fresh data: after a sync, a bounded filler of ordinary torch matmuls goes to
          `side`, an event is recorded, and the whole sequence is issued with no host
          synchronisation. Right after the first library call returns the filler's event must
          still be pending: the calls really were queued behind in-flight work. The filler is
          ten times the host-side enqueue time of the scenario's first call (the larger of two
          measurements on an idle stream with a warm context), capped at 200 ms, in whole
          matmuls; each run prints both figures (B2F_SIDE_STREAM_LOG=path appends them to a file).

  1  NTT and quotient table caches: more domains than slots, growing and stream-order-only reuse;
  2  pinned staging (the opening calls' blob, the permutation's instance table) reused back to back;
  3  the grand products' side streams: lookup, permutation, lookup with nothing between (two
     circuits, one group: no build can force the lookup's group below the circuit count);
  4  the commitments' and the IPA's shared scratch: long, MSM, short, long, fold;
  5  one proof-shaped chain, fill to commitments, and its one-bit fault;
  6  errors raised on the device survive b2f_sync on a side stream, 32 alternations (its syncs are
     the scenario: no filler);
  7  one context moved between streams with a sync between (likewise).

Needs an MI355X (`-m gpu`)."""
import math
import os
import random
import time

import numpy as np
import pytest

import ipa_ref as ir
import msm_ref as mr
import ntt_ref as nr
import open_ref as orf
import quotient_gates_ref as gr
import quotient_ref as qr

from conftest import random_inputs
from test_gpu_quotient import Problem, _block, _dev, _host, _pattern, _random_rows, _zeta

pytestmark = pytest.mark.gpu

FWD, INV = 0, 1
ERR_ARG, ERR_LAYOUT, ERR_FIELD = 1, 5, 7
ONES = np.uint64(2**64 - 1)
FILLER_N = 2048        # one filler unit: a [2048, 2048] fp32 matmul
FILLER_CAP_MS = 200.0
_filler = {}


def _side():
    import torch

    return torch.cuda.Stream()


def _filler_unit_ms(side):
    """Device time of one filler matmul, measured once per process (events around 50 of them)."""
    import torch

    if not _filler:
        a = torch.rand((FILLER_N, FILLER_N), device="cuda:0")
        out = torch.empty_like(a)
        torch.matmul(a, a, out=out)  # the first one loads the BLAS kernels
        side.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(side)
        for _ in range(50):
            torch.matmul(a, a, out=out)
        t1.record(side)
        t1.synchronize()
        _filler.update(a=a, out=out, unit_ms=t0.elapsed_time(t1) / 50)
    return _filler["unit_ms"]


def _log(line):
    print(line)
    path = os.environ.get("B2F_SIDE_STREAM_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def _cold_then_queued(name, prepare, issue, check):
    """prepare(engine, run) -> data (host references and device inputs; uploads block, so they all
    happen here); issue(engine, data, mark) -> outputs, calling mark() right after its first library call
    and returning at once if that answers True; check(data, outputs) reads back and compares."""
    import b2f
    import torch

    side = _side()
    eng = b2f.Engine(0)
    try:
        with torch.cuda.stream(side):
            s = side.cuda_stream
            unit = _filler_unit_ms(side)
            data = prepare(eng, 0)
            outs = issue(eng, data, lambda: False)
            eng.sync(s)
            check(data, outs)
            del outs
            # the first call's host-side enqueue time: idle stream, warm context
            took = []
            for _ in range(2):
                eng.sync(s)
                t0 = time.perf_counter()
                issue(eng, data, lambda: took.append(time.perf_counter() - t0) or True)
            enqueue_ms = 1e3 * max(took)
            data = prepare(eng, 1)
            eng.sync(s)
            filler_ms = min(10 * enqueue_ms, FILLER_CAP_MS)
            units = max(1, math.ceil(filler_ms / unit))
            for _ in range(units):
                torch.matmul(_filler["a"], _filler["a"], out=_filler["out"])
            filler_done = torch.cuda.Event()
            filler_done.record(side)
            seen = []
            outs = issue(eng, data, lambda: seen.append(filler_done.query()) and False)
            _log("side-stream %-8s first call enqueued in %.3f ms; filler %.3f ms = %d matmuls of %.3f ms; "
                 "filler pending after the first call: %s" % (name, enqueue_ms, units * unit, units, unit,
                                                               not seen[0]))
            assert seen == [False], "the first call returned after the filler had finished: nothing was queued"
            eng.sync(s)
            check(data, outs)
    finally:
        torch.cuda.synchronize()
        eng.close()


def _omega(form, k):
    from b2f import field

    return field.omega(field.of_form(form), k)


def _same(got, want, label):
    """uint64 limb arrays, bit for bit; names the first differing row."""
    got, want = np.asarray(got).reshape(-1, want.shape[-1]), np.asarray(want).reshape(-1, want.shape[-1])
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (label, "first differing row %d of %d" % (int(bad[0]), len(got)))


# ---------------------------------------------------------------------------------------------
# 1. the table caches


def _ntt_case(rng, form, k, direction, shift=None):
    p = nr.modulus(form)
    n = 1 << k
    shift = 2 + nr.random_elements(rng, 1, p - 2)[0] if shift is None else shift
    cols = [nr.random_elements(rng, n, p) for _ in range(3)]
    cols[0][0], cols[1][n - 1], cols[2][n // 2] = 0, p - 1, 1
    w = _omega(form, k)
    want = [nr.forward(c, k, w, shift, p) if direction == FWD else nr.inverse(c, k, w, shift, p) for c in cols]
    return dict(form=form, k=k, inverse=direction == INV, shift=shift,
                x=_dev(np.stack([nr.pack(c, form) for c in cols])),
                want=np.stack([nr.pack(c, form) for c in want]))


QUOT_SHAPES = [(1, 2, 1), (2, 5, 3), (3, 4, 1), (5, 7, 3), (4, 6, 1)]  # (k, ext_k, form): five ext_k, 4 slots


def _prepare_tables(eng, run):
    rng = np.random.default_rng(1100 + run)
    # ascending, forward, form 1: the ninth domain takes the first slot back and every slot grows;
    # descending, inverse, form 3: nine more domains, the last five into slots that are large enough
    # already (refilled by stream order alone); then the first domain again, long evicted
    ntt = [_ntt_case(rng, 1, k, FWD) for k in range(4, 13)]
    ntt += [_ntt_case(rng, 3, k, INV) for k in range(12, 3, -1)]
    ntt.append(_ntt_case(rng, 1, 4, FWD, shift=ntt[0]["shift"]))
    quot = []
    for k, ext_k, form in QUOT_SHAPES:
        pr = Problem(k, ext_k, form, 1200 + 10 * ext_k + run)
        usable, chunk = (1 << k) - 1, 3
        terms = qr.permutation_terms(k, ext_k, usable, pr.l, pr.v(), pr.sigma, pr.z[:3], chunk, pr.omega_ext,
                                     pr.shift, pr.delta, pr.beta, pr.gamma, pr.p)
        h = qr.fold(terms, pr.y, pr.p)
        quot.append(dict(pr=pr, usable=usable, chunk=chunk, z=pr.d_z[:3].contiguous(),
                         sel=np.stack([nr.pack(c, form) for c in qr.selectors(k, usable)]),
                         h=nr.pack(h, form),
                         q=nr.pack(qr.divide(h, k, ext_k, pr.omega_ext, pr.shift, pr.p), form)))
    return dict(ntt=ntt, quot=quot)


def _issue_tables(eng, data, mark):
    outs = []
    for i, c in enumerate(data["ntt"]):
        outs.append(eng.ntt_columns(c["x"], c["k"], inverse=c["inverse"], shift=c["shift"], form=c["form"]))
        if i == 0 and mark():
            return None
    for c in data["quot"]:
        pr = c["pr"]
        sel = eng.lagrange_selectors(pr.k, c["usable"], form=pr.form)
        h = eng.quotient_permutation(pr.k, pr.ext_k, c["usable"], pr.d_l, pr.d_adv, pr.d_sigma, c["z"], c["chunk"],
                                     pr.shift, pr.beta, pr.gamma, pr.y, form=pr.form)
        q = eng.quotient_divide(pr.k, pr.ext_k, pr.shift, h, out=h.new_empty(h.shape), form=pr.form)
        outs.append((sel, h, q))
    return outs


def _check_tables(data, outs):
    n_ntt = len(data["ntt"])
    for i, (c, out) in enumerate(zip(data["ntt"], outs)):
        _same(_host(out), c["want"], ("ntt", i, c["form"], c["k"], c["inverse"]))
    for c, (sel, h, q) in zip(data["quot"], outs[n_ntt:]):
        tag = (c["pr"].k, c["pr"].ext_k, c["pr"].form)
        _same(_host(sel), c["sel"], ("selectors",) + tag)
        _same(_host(h), c["h"], ("permutation terms",) + tag)
        _same(_host(q), c["q"], ("divide",) + tag)


def test_table_caches_cycle_without_a_sync():
    _cold_then_queued("tables", _prepare_tables, _issue_tables, _check_tables)


# ---------------------------------------------------------------------------------------------
# 2. pinned staging reused back to back

OPEN_N, OPEN_FORM, PERM_K = 4097, 1, 12
PERM_USABLE = (1 << PERM_K) - 7


def _perm_want(orc, adv, off, i0, i1, beta, gamma, chunk, form, sigma=True):
    import permutation as pm

    off = off[i0:i1 + 1].astype(np.int64)
    sig, zs = pm.columns(adv[:, int(off[0]):int(off[-1])], off - off[0], PERM_K, PERM_USABLE, beta, gamma, chunk,
                         nr.modulus(form), orc.copies)
    assert zs[-1][PERM_USABLE] == 1  # a valid trace closes
    return (np.stack([nr.pack(c, form) for c in sig]) if sigma else None,
            np.stack([nr.pack(c, form) for c in zs]))


def _oracle_trace(orc, x):
    ox = np.frombuffer(x.tobytes(), dtype=orc.INPUT_DTYPE).copy()
    adv, fixed, _, off = orc.fill(ox)
    return adv, fixed, off


def _staging_calls(r, p):
    """Eight calls, eight point sets and coefficient lists, the staged image shrinking and growing.
    r(count): fresh random elements."""
    return [
        ("eval", r(3), [(0, 0), (3, 2), (1, 1), (0, 2), (2, 0)]),
        ("combine", [[(0, r(1)[0]), (2, r(1)[0])], [(1, 1)]]),
        ("kate", [[r(1)[0]], [], r(2), [0, 1, p - 1]]),
        ("eval", r(12), [(c, q) for q in range(12) for c in (3, 0)]),
        ("combine", [[(c, v) for c, v in zip((0, 1, 2, 3, 0, 1, 2, 3), r(8))], [], [(3, p - 1)], [(2, r(1)[0])]]),
        ("kate", [r(12), r(1), [], r(5)]),
        ("eval", r(1), [(2, 0)]),
        ("kate", [r(3), r(3), r(3), r(3)]),
    ]


def _prepare_staging(orc, eng, run):
    import b2f

    form, n, p = OPEN_FORM, OPEN_N, nr.modulus(OPEN_FORM)
    rng = np.random.default_rng(1300 + run)
    cols = [nr.random_elements(rng, n, p) for _ in range(4)]
    cols[0][0], cols[1][n - 1], cols[3][n // 2] = 0, p - 1, 0
    r = lambda count: nr.random_elements(rng, count, p)  # noqa: E731
    calls = _staging_calls(r, p)
    want = []
    for call in calls:
        if call[0] == "eval":
            want.append(nr.pack([orf.eval(cols[c], call[1][q], p) for c, q in call[2]], form))
        elif call[0] == "combine":
            want.append(np.stack([nr.pack(orf.combine(cols, t, n, p), form) for t in call[1]]))
        else:
            want.append(np.stack([nr.pack(orf.divide_chain(cols[c], z, p), form) for c, z in enumerate(call[1])]))
    # two batches with different instance counts and rounds; the second brings a `rounds` the
    # context has not seen (another one in the queued run), so the pattern pool is rebuilt mid-sequence
    xa = random_inputs(2, (0,), 1310 + run)
    xa["rounds"] = np.asarray([0, 1], dtype=np.uint32)
    xb = random_inputs(3, (0,), 1320 + run)
    xb["rounds"] = np.asarray([1, 2 + run, 0], dtype=np.uint32)
    ch = r(6)
    ch[2], ch[3] = ch[2] % nr.modulus(3), ch[3] % nr.modulus(3)  # the second call's field is BN254's
    adv_a, _, off_a = _oracle_trace(orc, xa)
    adv_b, _, off_b = _oracle_trace(orc, xb)
    perm = [_perm_want(orc, adv_a, off_a, 0, 2, ch[0], ch[1], 3, 1),
            _perm_want(orc, adv_b, off_b, 0, 3, ch[2], ch[3], 5, 3),
            [_perm_want(orc, adv_b, off_b, a, b, ch[4], ch[5], 3, 1, sigma=False)[1] for a, b in ((0, 1), (1, 3))]]
    return dict(block=_block(cols, form, n), calls=calls, want=want, a=b2f.DeviceBatch(xa), b=b2f.DeviceBatch(xb),
                ch=ch, adv=(adv_a, adv_b), perm=perm)


def _issue_staging(eng, data, mark):
    outs, form = [], OPEN_FORM
    for i, call in enumerate(data["calls"]):
        if call[0] == "eval":
            outs.append(eng.poly_eval(data["block"], call[1], call[2], form=form))
        elif call[0] == "combine":
            outs.append(eng.poly_combine(data["block"], call[1], form=form))
        else:
            outs.append(eng.kate_divide(data["block"], call[1], form=form))
        if i == 0 and mark():
            return None
    a, b, ch = data["a"], data["b"], data["ch"]
    a.fill(eng)
    b.fill(eng)
    outs.append(a.permutation_columns(eng, PERM_K, PERM_USABLE, ch[0], ch[1], chunk_len=3, form=1))
    outs.append(b.permutation_columns(eng, PERM_K, PERM_USABLE, ch[2], ch[3], chunk_len=5, form=3))
    outs.append(b.permutation_columns_batch(eng, PERM_K, PERM_USABLE, ch[4], ch[5], [0, 1, 3], chunk_len=3, form=1))
    return outs


def _check_staging(data, outs):
    n_open = len(data["calls"])
    for i, (out, want) in enumerate(zip(outs, data["want"])):
        _same(_host(out), want, ("open call", i, data["calls"][i][0]))
    for batch, adv in zip((data["a"], data["b"]), data["adv"]):
        assert np.array_equal(batch.host_trace()[0], adv), "fill"
    for i in (0, 1):
        sig, z = outs[n_open + i]
        _same(_host(sig), data["perm"][i][0], ("sigma", i))
        _same(_host(z[:, :PERM_USABLE + 1]), data["perm"][i][1], ("z", i))
    zb = outs[n_open + 2]
    for c, want in enumerate(data["perm"][2]):
        _same(_host(zb[c, :, :PERM_USABLE + 1]), want, ("batch z, circuit", c))


def test_pinned_staging_reused_back_to_back(orc):
    _cold_then_queued("staging", lambda eng, run: _prepare_staging(orc, eng, run), _issue_staging, _check_staging)


# ---------------------------------------------------------------------------------------------
# 3. the grand products' side streams

LK_USABLE = 1 << 16  # the smallest circuit tests/test_gpu_lookup.py uses
LK_BEGINS = [0, 60000]
LK_PERM_K = 13       # one 12-round instance is 5,220 rows
_lk_trace = {}


def _prepare_fork_join(orc, eng, run):
    """The trace is the same in both runs (filled once, by the cold run's engine, with a sync). The
    two lookup calls differ in field and challenges, and the queued run issues them in the other
    order: each call follows one with other challenges, into output blocks that hold a pattern,
    and the 2^16-row references are computed once. The permutation's challenges are new each run."""
    import b2f
    import lookup as lk
    import permutation as pm
    import torch

    if "batch" not in _lk_trace:
        x = random_inputs(26, (12,), 61)
        _lk_trace["adv"], _, _lk_trace["off"] = _oracle_trace(orc, x)
        _lk_trace["batch"] = b2f.DeviceBatch(x)
        _lk_trace["batch"].fill(eng)
        eng.sync(torch.cuda.current_stream().cuda_stream)
        _lk_trace["begins"] = torch.tensor(LK_BEGINS, dtype=torch.int64, device="cuda:0")
    adv, off, batch = _lk_trace["adv"], _lk_trace["off"], _lk_trace["batch"]
    if "want" not in _lk_trace:
        rng = np.random.default_rng(1400)
        forms = (1, 3)  # pasta and BN254
        chal = [nr.random_elements(rng, 3, nr.modulus(f)) for f in forms]
        want = []
        for f, (theta, b, g) in zip(forms, chal):
            per = []
            for begin in LK_BEGINS:
                ref = lk.columns(adv[0, begin:begin + LK_USABLE], adv[1, begin:begin + LK_USABLE],
                                 adv[2, begin:begin + LK_USABLE], LK_USABLE, theta, b, g, nr.modulus(f))
                assert ref[4][-1] == 1  # a valid lookup closes
                per.append([nr.pack(col, f) for col in ref])
            want.append(per)
        _lk_trace.update(forms=forms, chal=chal, want=want)
    order = (0, 1) if run == 0 else (1, 0)
    forms, chal, want = ([_lk_trace[key][i] for i in order] for key in ("forms", "chal", "want"))
    beta, gamma = nr.random_elements(np.random.default_rng(1410 + run), 2, nr.P_PALLAS)
    usable = (1 << LK_PERM_K) - 7
    o = off[:2].astype(np.int64)
    sig, zs = pm.columns(adv[:, :int(o[1])], o, LK_PERM_K, usable, beta, gamma, 3, nr.P_PALLAS, orc.copies)
    assert zs[-1][usable] == 1
    return dict(batch=batch, forms=forms, chal=chal, want=want, beta=beta, gamma=gamma, usable=usable,
                sigma=np.stack([nr.pack(c, 1) for c in sig]), z=np.stack([nr.pack(c, 1) for c in zs]))


def _issue_fork_join(eng, data, mark):
    import torch

    batch = data["batch"]
    s = torch.cuda.current_stream().cuda_stream
    nc = len(LK_BEGINS)

    def lookup(i):
        out = torch.full((nc, 5, LK_USABLE + 1, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
        bad = torch.zeros(nc, dtype=torch.int64, device="cuda:0")
        theta, beta, gamma = data["chal"][i]
        # the begins are on the device already: DeviceBatch.lookup_columns would upload them (a
        # blocking copy) in front of the call
        eng.lookup_columns_dev(batch.advice.data_ptr(), batch.total_rows, _lk_trace["begins"].data_ptr(), nc,
                               LK_USABLE, theta, beta, gamma, data["forms"][i], out.data_ptr(), LK_USABLE + 1,
                               bad.data_ptr(), s)
        return out, bad

    first = lookup(0)
    if mark():
        return None
    perm = batch.permutation_columns(eng, LK_PERM_K, data["usable"], data["beta"], data["gamma"], chunk_len=3, form=1,
                                     instances=(0, 1))
    return first, perm, lookup(1)


def _check_fork_join(data, outs):
    first, (sig, z), second = outs
    for i, (out, bad) in enumerate((first, second)):
        assert (_host(bad) == ONES).all(), ("first_bad", i)
        h = _host(out)
        for c in range(len(LK_BEGINS)):
            for j, name in enumerate(["A", "S", "A'", "S'", "z"]):
                rows = LK_USABLE + 1 if j == 4 else LK_USABLE
                _same(h[c, j, :rows], data["want"][i][c][j], ("lookup call", i, "circuit", c, name))
    _same(_host(sig), data["sigma"], "sigma")
    _same(_host(z[:, :data["usable"] + 1]), data["z"], "permutation z")


def test_lookup_permutation_lookup_share_the_side_streams(orc):
    _lk_trace.clear()
    try:
        _cold_then_queued("forkjoin", lambda eng, run: _prepare_fork_join(orc, eng, run), _issue_fork_join,
                          _check_fork_join)
    finally:
        _lk_trace.clear()


# ---------------------------------------------------------------------------------------------
# 4. the scratch the commitments and the IPA rounds share

IPA_FORM, IPA_LONG, IPA_SHORT, MSM_LEN = 1, 1 << 12, 32, 3000


def _prepare_scratch(eng, run):
    form, cv = IPA_FORM, mr.curve_of_form(IPA_FORM)
    r = mr.ORDER[cv]
    rng = random.Random(1500 + run)
    gm, pts = mr.known_bases(form, IPA_LONG)
    vec, want = {}, {}
    for ln in (IPA_LONG, IPA_SHORT):
        p, b = [rng.randrange(r) for _ in range(ln)], [rng.randrange(r) for _ in range(ln)]
        vec[ln] = (p, b, _dev(mr.pack_scalars(form, p)), _dev(mr.pack_scalars(form, b)))
        want[ln] = (mr.pack_points(cv, ir.points_of(cv, ir.round_known(cv, p, gm[:ln]))),
                    mr.pack_scalars(form, ir.values(cv, p, b)))
    cols = [[rng.randrange(r) for _ in range(MSM_LEN)] for _ in range(5)]
    u = rng.randrange(1, r)
    p, b = vec[IPA_LONG][:2]
    p2, b2 = ir.fold_scalars(cv, p, b, u)
    half = IPA_LONG // 2
    idx = sorted({0, 1, 63, 64, 255, 256, half - 1} | set(rng.sample(range(half), 120)))
    g2 = ir.fold_known(cv, gm, u)
    return dict(g=_dev(mr.pack_points(cv, pts)), g_host=mr.pack_points(cv, pts), vec=vec, want=want, u=u, idx=idx,
                sc=_dev(np.stack([mr.pack_scalars(form, c) for c in cols])),
                msm=mr.pack_points(cv, [mr.expected_msm(form, c, gm[:MSM_LEN]) for c in cols]),
                p2=np.concatenate([mr.pack_scalars(form, p2), mr.pack_scalars(form, p[half:])]),
                b2=np.concatenate([mr.pack_scalars(form, b2), mr.pack_scalars(form, b[half:])]),
                g2=mr.pack_points(cv, ir.points_of(cv, [g2[i] for i in idx])))


def _issue_scratch(eng, data, mark):
    form, g = IPA_FORM, data["g"]

    def rnd(ln):
        return eng.ipa_round(data["vec"][ln][2], data["vec"][ln][3], g, len=ln, form=form)

    outs = [rnd(IPA_LONG)]
    if mark():
        return None
    outs.append(eng.msm(data["sc"], g, len=MSM_LEN, form=form))
    outs.append(rnd(IPA_SHORT))
    outs.append(rnd(IPA_LONG))
    eng.ipa_fold(data["vec"][IPA_LONG][2], data["vec"][IPA_LONG][3], g, data["u"], len=IPA_LONG, form=form)
    return outs


def _check_scratch(data, outs):
    for i, ln in ((0, IPA_LONG), (2, IPA_SHORT), (3, IPA_LONG)):
        lr, vals = outs[i]
        _same(_host(lr), data["want"][ln][0], ("L, R of call", i))
        _same(_host(vals), data["want"][ln][1], ("values of call", i))
    _same(_host(outs[1]), data["msm"], "commitments")
    half = IPA_LONG // 2
    _same(_host(data["vec"][IPA_LONG][2]), data["p2"], "folded p, and its upper half untouched")
    _same(_host(data["vec"][IPA_LONG][3]), data["b2"], "folded b, and its upper half untouched")
    hg = _host(data["g"])
    _same(hg[data["idx"]], data["g2"], "folded G")
    _same(hg[half:], data["g_host"][half:], "G's upper half untouched")


def test_commitment_and_ipa_scratch_long_short_long():
    _cold_then_queued("scratch", _prepare_scratch, _issue_scratch, _check_scratch)


# ---------------------------------------------------------------------------------------------
# 5. one proof-shaped chain


def _prepare_chain(eng, run):
    import b2f
    from b2f import field

    form, k = 1, 10
    p = nr.modulus(form)
    x = random_inputs(2, (0,), 1600 + run)
    x["rounds"] = np.asarray([1, 0], dtype=np.uint32)
    rng = np.random.default_rng(1610 + run)
    y, xp = nr.random_elements(rng, 2, p)
    gm, pts = mr.known_bases(form, 1 << k)
    return dict(batch=b2f.DeviceBatch(x), y=y, xp=xp, gm=gm, bases=_dev(mr.pack_points(mr.curve_of_form(form), pts)),
                queries=[tuple(int(v) for v in row) for row in b2f.gate_queries()],
                points=field.rotated_points(field.of_form(form), xp, k, range(12)), seed=1620 + run)


def _issue_chain(eng, data, mark):
    import b2f
    import torch

    form, k, ext_k = 1, 10, 12
    n, shift = 1 << k, _zeta(form)
    batch = data["batch"]
    batch.fill(eng)
    if mark():
        return None
    used = int(batch.offsets_host[-1])
    adv = torch.zeros((10, n, 4), dtype=torch.int64, device="cuda:0")
    fixed = torch.zeros((17, n, 4), dtype=torch.int64, device="cuda:0")
    batch.export_fp(eng, 0, used, form=form, out=adv)
    batch.export_fixed_fp(eng, 0, used, form=form, out=fixed)
    adv[:, used:] = _random_rows((10, n - used, 4), data["seed"])  # blinding rows
    fixed_c = eng.ntt_columns(fixed, k, inverse=True, form=form)
    fixed_e = eng.ntt_columns(fixed_c, ext_k, shift=shift, in_len=n, form=form)
    fixed_x = eng.poly_eval(fixed_c, [data["xp"]], [(g, 0) for g in range(17)], form=form)

    def sides(advice):
        adv_c = eng.ntt_columns(advice, k, inverse=True, form=form)
        adv_e = eng.ntt_columns(adv_c, ext_k, shift=shift, in_len=n, form=form)
        h = eng.quotient_gates(k, ext_k, adv_e, fixed_e, data["y"], form=form)
        h = eng.quotient_divide(k, ext_k, shift, h, form=form)
        coeff = eng.ntt_columns(h[None], ext_k, inverse=True, shift=shift, form=form)
        pieces = coeff.reshape(4, n, 4)  # the h pieces: columns of stride n
        h_x = eng.poly_eval(pieces, [data["xp"]], [(i, 0) for i in range(4)], form=form)
        a_x = eng.poly_eval(adv_c, data["points"], data["queries"], form=form)
        return pieces, h_x, a_x, eng.msm(pieces, data["bases"], form=form)

    good = sides(adv)
    bad = adv.clone()
    bad[b2f.halo2_column_index(9), 164, 0] ^= 1  # the carry of the first ADD3 block, as in the quotient test
    return fixed_x, good, sides(bad)


def _check_chain(data, outs):
    form, n = 1, 1 << 10
    p = nr.modulus(form)
    unpack = lambda t: nr.unpack(_host(t).reshape(-1, 4), form)  # noqa: E731
    fixed_x, good, bad = outs
    fixed_x = unpack(fixed_x)
    xp, y = data["xp"], data["y"]

    def identity(pieces, h_x, a_x, commitments):
        h_x, a_x = unpack(h_x), dict(zip(data["queries"], unpack(a_x)))
        xn = pow(xp, n, p)
        left = (xn - 1) * sum(pow(xn, i, p) * v for i, v in enumerate(h_x)) % p
        right = 0
        for g in range(16):
            polys = [a_x[(gr.HALO2[1], 0)] - fixed_x[16]] if g == 14 else gr.GATES[g](lambda c, j: a_x[(gr.HALO2[c], j)])
            for poly in polys:
                right = (right * y + fixed_x[g] * poly) % p
        # the commitments of the four pieces, and the pieces' own evaluations, from the coefficients
        cv = mr.curve_of_form(form)
        coeffs = [unpack(c) for c in pieces]
        assert h_x == [orf.eval(c, xp, p) for c in coeffs]
        _same(_host(commitments), mr.pack_points(cv, [mr.expected_msm(form, c, data["gm"]) for c in coeffs]),
              "commitments of the h pieces")
        return left, right

    left, right = identity(*good)
    assert left == right and left != 0
    left, right = identity(*bad)
    assert left != right


def test_proof_shaped_chain_from_fill_to_commitments():
    _cold_then_queued("chain", _prepare_chain, _issue_chain, _check_chain)


# ---------------------------------------------------------------------------------------------
# 6. errors survive b2f_sync on a side stream

ALTERNATIONS = 32


def _alternate(bad_call, good_call, code):
    """A fresh engine whose very first call is the bad one, on `side`; then good + sync (clean, right
    result) and bad + sync (raises) in turn. Nothing here faults the GPU: these are the library's
    own flags."""
    import b2f
    import torch

    side = _side()
    eng = b2f.Engine(0)
    try:
        with torch.cuda.stream(side):
            s = side.cuda_stream
            bad_call(eng, s)
            with pytest.raises(b2f.B2FError) as e:
                eng.sync(s)
            assert e.value.code == code, "the very first call"
            for i in range(ALTERNATIONS):
                check = good_call(eng, s)
                eng.sync(s)  # the previous error was cleared, and stays cleared
                check(i)
                bad_call(eng, s)
                with pytest.raises(b2f.B2FError) as e:
                    eng.sync(s)  # a late clear of the previous sync would have swallowed this one
                assert e.value.code == code, i
            check = good_call(eng, s)
            eng.sync(s)
            check(ALTERNATIONS)
    finally:
        torch.cuda.synchronize()
        eng.close()


def _ntt_pair():
    """The inputs of test_gpu_ntt.py::test_a_generator_of_the_wrong_order_raises_at_sync."""
    form, k = 2, 9
    p, n = nr.modulus(form), 1 << 9
    rng = np.random.default_rng(81)
    vals = nr.random_elements(rng, n, p)
    shift = 2 + nr.random_elements(rng, 1, p - 2)[0]
    d_in, d_pat = _dev(nr.pack(vals, form)[None]), _dev(_pattern((1, n, 4)))
    want = nr.pack(nr.forward(vals, k, _omega(form, k), shift, p), form)

    def run(eng, s, omega):
        out = d_pat.clone()
        eng.ntt_columns_dev(d_in.data_ptr(), n, n, 1, k, omega, shift, FWD, form, out.data_ptr(), n, s)
        return out

    def good(eng, s):
        out = run(eng, s, _omega(form, k))
        return lambda i: _same(_host(out), want[None].reshape(-1, 4), ("good ntt", i))

    return (lambda eng, s: run(eng, s, _omega(form, k - 1))), good


def test_wrong_root_raises_at_every_sync_on_a_side_stream():
    import torch

    with torch.cuda.stream(_side()):  # the uploads too
        bad, good = _ntt_pair()
    _alternate(bad, good, ERR_FIELD)


def test_vanishing_point_raises_at_every_sync_on_a_side_stream():
    import torch

    form, k, ext_k = 1, 3, 5
    with torch.cuda.stream(_side()):
        pr = Problem(k, ext_k, form, 451)
        h_in = _block([pr.h_in], form, pr.rows)[0]
    want = nr.pack(qr.divide(pr.h_in, k, ext_k, pr.omega_ext, pr.shift, pr.p), form)

    def divide(eng, s, shift):
        out = torch.empty_like(h_in)
        eng.quotient_divide_dev(k, ext_k, pr.omega_ext, shift, h_in.data_ptr(), out.data_ptr(), form, s)
        return out

    def good(eng, s):
        out = divide(eng, s, pr.shift)
        return lambda i: _same(_host(out)[:pr.n_ext], want, ("good divide", i))

    _alternate(lambda eng, s: divide(eng, s, 1), good, ERR_FIELD)  # shift = 1: X_0^n = 1


def test_rejected_row_map_raises_at_every_sync_on_a_side_stream(orc):
    import b2f
    import torch

    x = random_inputs(6, (1, 2, 4), 10)
    adv, fixed, off = _oracle_trace(orc, x)
    want = orc.evaluate(adv, fixed, off)
    assert want["first_failure"] == 2**64 - 1
    with torch.cuda.stream(_side()):
        batch = b2f.DeviceBatch(x)
        batch.advice.copy_(torch.from_numpy(adv.view(np.int32)))  # the oracle's trace: no fill call comes first
        batch.fixed.copy_(torch.from_numpy(fixed.view(np.int32)))
        good_off = batch.offsets.clone()
        bad_off = good_off.clone()
        bad_off[3] += 4  # not a LAYOUT v1 prefix sum any more
        torch.cuda.current_stream().synchronize()

    def evaluate(eng, s, offsets):
        eng.eval_dev(batch.advice.data_ptr(), batch.fixed.data_ptr(), offsets.data_ptr(), batch.n, batch.total_rows,
                     batch.report.data_ptr(), s)

    def good(eng, s):
        evaluate(eng, s, good_off)

        def check(i):
            assert batch.report_dict() == want, i  # under the side stream's context: it synchronises that stream

        return check

    _alternate(lambda eng, s: evaluate(eng, s, bad_off), good, ERR_LAYOUT)


def test_refused_argument_on_a_side_stream_opens_no_region():
    import b2f
    import torch

    side = _side()
    eng = b2f.Engine(0)
    try:
        with torch.cuda.stream(side):
            s = side.cuda_stream
            _, good = _ntt_pair()
            eng.set_timing(True)
            with pytest.raises(b2f.B2FError) as e:
                eng.ntt_columns_dev(0, 512, 512, 1, 9, _omega(2, 9), 1, FWD, 2, 0, 512, s)
            assert e.value.code == ERR_ARG
            check = good(eng, s)
            eng.sync(s)
            check(0)
            times = eng.kernel_times()
            assert times["ntt"][1] == 1 and times["ntt"][0] > 0
            assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "ntt")
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---------------------------------------------------------------------------------------------
# 7. one context, three streams, a sync between


def test_moving_a_context_between_streams_with_a_sync_between():
    import b2f
    import torch

    form, k, n = 3, 11, 1 << 11  # two NTT passes
    p = nr.modulus(form)
    rng = np.random.default_rng(1700)
    cols = [nr.random_elements(rng, n, p) for _ in range(2)]
    shift = 2 + nr.random_elements(rng, 1, p - 2)[0]
    pts = nr.random_elements(rng, 3, p)
    queries = [(1, 2), (0, 0), (0, 1), (1, 0)]
    want_ntt = np.stack([nr.pack(nr.forward(c, k, _omega(form, k), shift, p), form) for c in cols])
    want_ev = nr.pack([orf.eval(cols[c], pts[q], p) for c, q in queries], form)
    eng = b2f.Engine(0)
    try:
        eng.set_timing(True)
        results = []
        for stream in (_side(), _side(), torch.cuda.default_stream()):
            with torch.cuda.stream(stream):
                s = torch.cuda.current_stream().cuda_stream
                assert s == stream.cuda_stream
                block = _block(cols, form, n)  # a fresh upload on this stream
                out = eng.ntt_columns(block, k, shift=shift, form=form)
                ev = eng.poly_eval(block, pts, queries, form=form)
                eng.sync(s)  # what a caller owes before the context moves to another stream
                times = eng.kernel_times()
                assert times["ntt"][1] == 1 and times["ntt"][0] > 0, s
                assert times["quotient"][1] == 1 and times["quotient"][0] > 0, s
                assert all(cnt == 0 for name, (_, cnt) in times.items() if name not in ("ntt", "quotient")), s
                results.append((_host(out), _host(ev)))
        for i, (out, ev) in enumerate(results):
            _same(out, want_ntt, ("ntt on stream", i))
            _same(ev, want_ev, ("poly_eval on stream", i))
    finally:
        torch.cuda.synchronize()
        eng.close()
