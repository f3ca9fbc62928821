"""b2f_msm_dev (csrc/b2f_msm.hip) against the big-integer reference of tests/msm_ref.py, bit for
bit, on both curves. The bases are known multiples b_i G of the generator, so the expected output
of any case is the one scalar multiplication (sum s_i b_i mod r) G; for len <= 64 the sum is also
formed point by point (bitwise_msm), so that not everything rests on that formula.

  1  small lengths x forms: every len in 1..67, 127..129, 255..257, 1023..1025, 4097 (Montgomery
     forms; canonical forms up to 257), 3 columns with 0, 1 and p - 1 in chosen cells, rows =
     len + 5 with the pad rows all ones, inputs unchanged afterwards;
  2  forced window widths c in {1, 2, 5, 8, 13, 16} (diagnostics library) on scalars built for the
     recoding: p - 1, 2^k - 1 around every window edge, every digit 2^c - 1 (a full carry chain),
     every digit 2^(c-1), the largest scalars with a carry out of each of the top windows;
  3  degenerate bases: all equal (every bucket addition an equal-point case), G and -G alternating
     with pairwise equal scalars (all zeros out), some (0, 0) bases, all-zero scalars, one non-zero
     scalar at the first, a middle and the last row;
  4  scalar distributions at len = 2^16 + 3 in one call: all ones, one repeated large value, 0/1,
     a real advice column of the chip, uniform random;
  5  len = 2^17 + 5 with the incremental base family; 5 columns in one call = five calls; forced
     group 2 with 5 and 7 columns; a forced c = 1 whose digits exceed a pass (row chunks);
  6  scratch reuse: large, small, large on one engine with different data;
  7  every refused argument, a good call after each, and the call's timing region.

Needs an MI355X (`-m gpu`). No test passes the device anything the host does not check first."""
import os
import random

import numpy as np
import pytest

import msm_ref as mr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ROWS = 1, 3
BIG = (1 << 17) + 5
ONES = np.uint64(0xffffffffffffffff)


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _scalar_block(form, cols, rows):
    """cols: lists of ints (len each) -> uint64 [n_cols, rows, 4] in `form`, rows past len all ones."""
    ln = len(cols[0])
    blk = np.full((len(cols), rows, 4), ONES, dtype=np.uint64)
    for c, col in enumerate(cols):
        assert len(col) == ln
        blk[c, :ln] = mr.pack_scalars(form, col)
    return blk


def _msm(eng, form, cols, pts, rows=None, extra_bases=0):
    """One call on int columns and affine bases; returns the affine outputs. Checks that the call
    leaves its inputs as they were."""
    import torch

    cv = mr.curve_of_form(form)
    ln = len(cols[0])
    rows = ln if rows is None else rows
    d_sc = _dev(_scalar_block(form, cols, rows))
    d_b = _dev(mr.pack_points(cv, list(pts) + [mr.GEN[cv]] * extra_bases))
    sc0, b0 = d_sc.clone(), d_b.clone()
    out = eng.msm(d_sc, d_b, len=ln, form=form)
    eng.sync(torch.cuda.current_stream().cuda_stream)
    assert torch.equal(d_sc, sc0) and torch.equal(d_b, b0), "the call changed an input"
    return mr.unpack_points(cv, out.cpu().numpy())


def _expect(form, cols, multiples):
    return [mr.expected_msm(form, col, multiples) for col in cols]


def _small_cols(cv, ln, seed):
    r = mr.ORDER[cv]
    rng = random.Random(seed)
    cols = [[rng.randrange(r) for _ in range(ln)] for _ in range(3)]
    for c, v in enumerate((0, 1, r - 1)):  # in chosen cells: first, last, middle, rotated by column
        cols[c][0] = v
        cols[(c + 1) % 3][ln - 1] = v
        cols[(c + 2) % 3][ln // 2] = v
    return cols


SMALL_LENS = list(range(1, 68)) + [127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097]
_naive_cache = {}


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_small_lengths_and_forms(engine, form):
    cv = mr.curve_of_form(form)
    for ln in SMALL_LENS:
        if not form & 1 and ln > 257:
            continue
        bs, pts = mr.known_bases(form, ln)
        cols = _small_cols(cv, ln, 100 + ln)
        got = _msm(engine, form, cols, pts, rows=ln + 5, extra_bases=ln % 3)
        assert got == _expect(form, cols, bs), (form, ln)
        if ln <= 64:  # column 0 point by point (the same scalars for both forms of a curve)
            if (cv, ln) not in _naive_cache:
                _naive_cache[cv, ln] = mr.bitwise_msm(cv, cols[0], pts)
            assert got[0] == _naive_cache[cv, ln], (form, ln)


def _recoding_scalars(cv, c):
    r = mr.ORDER[cv]
    out = [r - 1, r - 2, 0, 1]
    for edge in range(0, 256 + c, c):
        for k in (edge - 1, edge, edge + 1):
            if 0 < k and (1 << k) - 1 < r:
                out.append((1 << k) - 1)
    top = 0
    while (1 << (c * (top + 1))) - 1 < r:
        top += 1
    out.append((1 << (c * top)) - 1)  # every digit 2^c - 1: the carry runs through all windows
    half = 0
    for w in range(256 // c + 1):
        if half + (1 << (c - 1) << (w * c)) < r:
            half += 1 << (c - 1) << (w * c)
    out.append(half)  # every digit exactly 2^(c-1): the largest digit that does not borrow
    for w in range(max(0, 253 // c - 3), 256 // c + 1):  # the largest scalars carrying out of window w
        hi = ((r - 1) >> ((w + 1) * c)) << ((w + 1) * c)
        if hi:
            out.append(hi - 1)
    return out


@pytest.mark.parametrize("c", [1, 2, 5, 8, 13, 16])
def test_forced_window_widths_and_carries(diag_engine, c):
    from b2f import _lib

    ln = 300
    assert "B2F_DIAG_MSM_PLAN" not in os.environ
    try:
        os.environ["B2F_DIAG_MSM_PLAN"] = str(c)
        assert _lib.msm_plan(ln, 1, 1, diag=True)["window_bits"] == c
        for form in (1, 3):
            cv = mr.curve_of_form(form)
            rng = random.Random(200 + c + form)
            sp = _recoding_scalars(cv, c)
            n_cols = -(-len(sp) // ln)
            sp += [rng.randrange(mr.ORDER[cv]) for _ in range(n_cols * ln - len(sp))]
            cols = [sp[i * ln:(i + 1) * ln] for i in range(n_cols)]
            bs, pts = mr.known_bases(form, ln)
            assert _msm(diag_engine, form, cols, pts) == _expect(form, cols, bs), (c, form)
    finally:
        os.environ.pop("B2F_DIAG_MSM_PLAN", None)


@pytest.mark.parametrize("form", [1, 3])
def test_degenerate_bases(engine, form):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(300 + form)
    ln = 200
    g = mr.GEN[cv]
    rand = [rng.randrange(r) for _ in range(ln)]
    small = [rng.randrange(1, 4) for _ in range(ln)]  # few buckets: long equal-point chains
    # all bases equal: every bucket addition adds a point to a multiple of itself
    b7 = mr.gen_mul(cv, 7)
    assert _msm(engine, form, [rand, small, [1] * ln], [b7] * ln) == _expect(form, [rand, small, [1] * ln], [7] * ln)
    # G, -G alternating, scalars equal in pairs: every output is the identity, all zeros
    pair = [rand[i // 2] for i in range(ln)]
    pair_small = [small[i // 2] for i in range(ln)]
    alt = [g if i % 2 == 0 else mr.neg(cv, g) for i in range(ln)]
    assert _msm(engine, form, [pair, pair_small], alt) == [None, None]
    # some bases (0, 0)
    bs, pts = mr.known_bases(form, ln)
    bs, pts = list(bs), list(pts)
    for i in (0, 1, 57, 58, 59, ln - 1):
        bs[i], pts[i] = 0, None
    assert _msm(engine, form, [rand, small], pts) == _expect(form, [rand, small], bs)
    assert _msm(engine, form, [rand], [None] * ln) == [None]
    # all scalars zero; exactly one non-zero scalar at the first, a middle and the last row
    bs, pts = mr.known_bases(form, ln)
    cols = [[0] * ln]
    for at in (0, 101, ln - 1):
        col = [0] * ln
        col[at] = rand[at] or 1
        cols.append(col)
    got = _msm(engine, form, cols, pts)
    assert got[0] is None and got == _expect(form, cols, bs)
    assert got[1] == mr.mul(cv, cols[1][0], pts[0])


def _advice_column(engine, ln):
    """A real advice column of the chip as canonical ints: a small filled batch exported with
    export_fp (Montgomery form), limbs unpacked on the host."""
    import torch

    import b2f
    from b2f import synth

    x = synth.batch(14, rounds_mix=[12])
    batch = b2f.DeviceBatch(x, device="cuda:0")
    assert batch.used_rows >= ln
    batch.fill(engine)
    # halo2 column 8 is a_1, the dense 16-bit limbs of the spread lookups
    col = batch.export_fp(engine, 0, ln, form=b2f.FP_MONTGOMERY)[b2f.halo2_column_index(1)].contiguous()
    engine.sync(torch.cuda.current_stream().cuda_stream)
    raw = col.cpu().numpy().view(np.uint64).tobytes()
    p = mr.ORDER[0]
    rinv = pow(mr.R, -1, p)
    vals = [int.from_bytes(raw[i:i + 32], "little") * rinv % p for i in range(0, len(raw), 32)]
    print("advice column: %d distinct values in %d rows, largest %d bits"
          % (len(set(vals)), len(vals), max(vals).bit_length()))
    assert len(vals) == ln and len(set(vals)) > 1
    return vals


@pytest.mark.parametrize("form", [1, 3])
def test_scalar_distributions(engine, form):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    ln = (1 << 16) + 3
    rng = random.Random(400 + form)
    bs, pts = mr.known_bases(form, BIG, incremental=True)
    bs, pts = bs[:ln], pts[:ln]
    big = rng.randrange(r >> 1, r)
    cols = [[1] * ln, [big] * ln, [rng.randrange(2) for _ in range(ln)], _advice_column(engine, ln),
            [rng.randrange(r) for _ in range(ln)]]
    got = _msm(engine, form, cols, pts)
    assert got == _expect(form, cols, bs)
    assert got[0] == mr.gen_mul(cv, sum(bs) % r)  # the all-ones column is the sum of the bases


@pytest.mark.parametrize("form", [1, 3])
def test_size_and_batching(engine, diag_engine, form):
    from b2f import _lib

    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(500 + form)
    bs, pts = mr.known_bases(form, BIG, incremental=True)
    cols = [[rng.randrange(r) for _ in range(BIG)] for _ in range(3)]
    assert _msm(engine, form, cols, pts) == _expect(form, cols, bs)
    # 5 columns in one call = five single-column calls (and the reference)
    ln = 3001
    cols = [[rng.randrange(r) for _ in range(ln)] for _ in range(7)]
    want = _expect(form, cols, bs[:ln])
    assert _msm(engine, form, cols[:5], pts[:ln]) == want[:5]
    assert [_msm(engine, form, [c], pts[:ln])[0] for c in cols[:5]] == want[:5]
    assert "B2F_DIAG_MSM_PLAN" not in os.environ
    try:
        c = _lib.msm_plan(ln, 5, form)["window_bits"]
        os.environ["B2F_DIAG_MSM_PLAN"] = "%d,2" % c
        assert _lib.msm_plan(ln, 7, form, diag=True)["group"] == 2
        assert _msm(diag_engine, form, cols[:5], pts[:ln]) == want[:5]
        assert _msm(diag_engine, form, cols, pts[:ln]) == want
        # c = 1: 256 digits a scalar, more than one pass holds at this length: rows go in chunks
        os.environ["B2F_DIAG_MSM_PLAN"] = "1"
        col = [rng.randrange(r) for _ in range(BIG)]
        assert _msm(diag_engine, form, [col], pts) == _expect(form, [col], bs)
    finally:
        os.environ.pop("B2F_DIAG_MSM_PLAN", None)


@pytest.mark.parametrize("form", [1, 3])
def test_scratch_reuse(form):
    import b2f

    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(600 + form)
    eng = b2f.Engine(0)
    try:
        bs, pts = mr.known_bases(form, 20000)
        for ln, n_cols in ((20000, 2), (5, 1), (19999, 2), (1, 3)):
            cols = [[rng.randrange(r) for _ in range(ln)] for _ in range(n_cols)]
            assert _msm(eng, form, cols, pts[:ln]) == _expect(form, cols, bs[:ln]), ln
    finally:
        eng.close()


def test_refused_arguments_and_timing(engine):
    import torch

    from b2f import B2FError

    form, ln, rows = 1, 40, 48
    cv = 0
    rng = random.Random(700)
    bs, pts = mr.known_bases(form, ln)
    cols = [[rng.randrange(mr.ORDER[cv]) for _ in range(ln)] for _ in range(2)]
    want = _expect(form, cols, bs)
    d_sc = _dev(_scalar_block(form, cols, rows))
    d_b = _dev(mr.pack_points(cv, pts))
    d_out = torch.zeros((2, 8), dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    S, Bp, O = d_sc.data_ptr(), d_b.data_ptr(), d_out.data_ptr()

    def good():
        d_out.zero_()
        engine.msm_dev(S, rows, ln, 2, Bp, ln, form, O, s)
        engine.sync(s)
        assert mr.unpack_points(cv, d_out.cpu().numpy()) == want

    good()
    refused = [
        (ERR_ARG, (0, rows, ln, 2, Bp, ln, form, O)), (ERR_ARG, (S, rows, ln, 2, 0, ln, form, O)),
        (ERR_ARG, (S, rows, ln, 2, Bp, ln, form, 0)),
        (ERR_ARG, (S + 8, rows, ln, 2, Bp, ln, form, O)), (ERR_ARG, (S, rows, ln, 2, Bp + 8, ln, form, O)),
        (ERR_ARG, (S, rows, ln, 2, Bp, ln, form, O + 8)),
        (ERR_ARG, (S, rows, ln, 2, Bp, ln, 4, O)),
        (ERR_ARG, (S, rows, 0, 2, Bp, ln, form, O)),
        (ERR_ARG, (S, (1 << 28) + 8, (1 << 28) + 1, 2, Bp, (1 << 28) + 1, form, O)),
        (ERR_ARG, (S, rows, ln, 0, Bp, ln, form, O)),
        (ERR_ARG, (S, rows, ln, 2, Bp, ln, form, S)),        # the output on the scalars
        (ERR_ARG, (S, rows, ln, 2, Bp, ln, form, S + 64)),
        (ERR_ARG, (S, rows, ln, 2, Bp, ln, form, Bp + 64 * (ln - 1))),  # ... on the last base
        (ERR_ROWS, (S, ln - 1, ln, 2, Bp, ln, form, O)),     # len > rows
        (ERR_ROWS, (S, rows, ln, 2, Bp, ln - 1, form, O)),   # len > n_bases
    ]
    for code, args in refused:
        with pytest.raises(B2FError) as e:
            engine.msm_dev(*args, s)
        assert e.value.code == code, args
        good()
    engine.set_timing(True)
    engine.msm_dev(S, rows, ln, 2, Bp, ln, form, O, s)
    times = engine.kernel_times()
    engine.set_timing(False)
    assert times["quotient"][1] == 1 and times["quotient"][0] > 0
    assert all(v[1] == 0 for k, v in times.items() if k != "quotient")
