"""b2f_msm_cells_dev (csrc/b2f_msm.hip: columns committed from their u32 cells, plus a tail of
full scalars) against the big-integer reference of tests/msm_ref.py, bit for bit, on both curves.
The bases are known multiples b_i G, so the expectation of a column is (sum s_i b_i mod r) G with
s the scalars tests/cells_ref.py cuts from the cells; for len <= 64 the sum is also formed point
by point (bitwise_msm).

  1  small lengths: every len in 1..67, 127..129, 255..257, 1023..1025, 4097; six columns of
     (shift, bits) = (0,32) (0,16) (16,16) (0,1) (7,1) (3,17) at offsets that are no multiple of 4,
     one with avail = len - 1, one with avail = 0, one with avail > len; chosen values first, middle
     and last; every cell outside a column's rows and every bit outside its field all ones;
  2  forced window widths c in {1, 2, 5, 8, 13, 16} (diagnostics library) on cells built for the
     recoding;
  3  the tail: 1, 6 and 64 rows in all four forms, len = 1, and no tail;
  4  a real trace filled by the fused pass: three circuits in one commit_advice call against
     b2f_msm_dev on the exported block (on the device) and the big integers; commit_fixed;
  5  distributions at len = 2^16 + 3 in one call;
  6  len = 2^17 + 5; 5 columns in one call = five calls; forced group 2; a forced c = 1 at
     len = 2^19 + 3 (33 windows, two row chunks);
  7  the scratch shared with b2f_msm_dev and the IPA round;
  8  every refused argument, a good call after each, and the call's timing region.

Needs an MI355X (`-m gpu`). No test passes the device anything the host does not check first."""
import os
import random

import numpy as np
import pytest

import cells_ref as cr
import ipa_ref as ir
import msm_ref as mr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ROWS = 1, 3
BIG = (1 << 17) + 5
ALL = 0xffffffff
PLANTED = [0, ALL, 0x80000000, 0x8000, 0xffff, 0x10000]
SHAPES = [(0, 32), (0, 16), (16, 16), (0, 1), (7, 1), (3, 17)]


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _dev_cells(cells):
    import torch

    return torch.from_numpy(np.ascontiguousarray(cells, dtype=np.uint32).view(np.int32)).to("cuda:0")


_packed_pool = {}


def _bases(form, n, incremental=False):
    """(multiples, device points): the incremental family, or the pool cycled (packed once)."""
    cv = mr.curve_of_form(form)
    if incremental:
        bs, pts = mr.known_bases(form, n, incremental=True)
        return bs, _dev(mr.pack_points(cv, pts))
    if cv not in _packed_pool:
        bs, pts = mr.known_bases(form, mr.POOL_SIZE)
        _packed_pool[cv] = (bs, mr.pack_points(cv, pts))
    bs, packed = _packed_pool[cv]
    reps = -(-n // mr.POOL_SIZE)
    return (bs * reps)[:n], _dev(np.tile(packed, (reps, 1))[:n])


def _tail_block(form, tail):
    return None if not tail else _dev(np.stack([mr.pack_scalars(form, t) for t in tail]))


def _expect(form, cells, cols, ln, bs, tail=None):
    out = []
    for j, col in enumerate(cols):
        sc = cr.column_scalars(cells, col, ln) + (list(tail[j]) if tail else [])
        out.append(mr.expected_msm(form, sc, bs))
    return out


def _call(eng, form, cells, cols, ln, d_bases, tail=None):
    """One call; returns the affine outputs. Checks that the call leaves its inputs as they were."""
    import torch

    d_cells, d_tail = _dev_cells(cells), _tail_block(form, tail)
    c0, b0 = d_cells.clone(), d_bases.clone()
    t0 = None if d_tail is None else d_tail.clone()
    out = eng.msm_cells(d_cells, cols, d_bases, ln, tail=d_tail, form=form)
    eng.sync(torch.cuda.current_stream().cuda_stream)
    assert torch.equal(d_cells, c0) and torch.equal(d_bases, b0), "the call changed an input"
    assert t0 is None or torch.equal(d_tail, t0), "the call changed the tail"
    return mr.unpack_points(mr.curve_of_form(form), out.cpu().numpy())


def _layout(ln, values, avails):
    """Cells all ones except each column's field in its first avail rows; offsets no multiple of 4."""
    cols, at = [], 1
    for (shift, bits), avail in zip(SHAPES, avails):
        while at % 4 == 0:
            at += 1
        cols.append((at, avail, shift, bits))
        at += ln + 2
    cells = np.full(at + 8, ALL, dtype=np.uint32)
    for (offset, avail, shift, bits), vals in zip(cols, values):
        mask = (1 << bits) - 1
        for i in range(min(avail, ln)):
            cells[offset + i] = (ALL ^ (mask << shift)) | ((vals[i] & mask) << shift)
    return cells, cols


SMALL_LENS = list(range(1, 68)) + [127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097]
_naive_cache = {}


@pytest.mark.parametrize("form", [1, 3])
def test_small_lengths(engine, form):
    cv = mr.curve_of_form(form)
    for ln in SMALL_LENS:
        rng = random.Random(100 + ln)
        values = [[rng.randrange(1 << 32) for _ in range(ln)] for _ in SHAPES]
        for j in range(6):
            for k, at in enumerate((0, ln // 2, ln - 1)):
                values[j][at] = PLANTED[(j + 2 * k) % 6]
        avails = [ln, ln - 1, ln + 2, ln, 0, ln]
        cells, cols = _layout(ln, values, avails)
        bs, d_b = _bases(form, ln + ln % 3)
        got = _call(engine, form, cells, cols, ln, d_b)
        want = _expect(form, cells, cols, ln, bs)
        assert got == want, (form, ln)
        assert got[4] is None, "avail = 0 is the identity"
        # the model cut what was planted: the field of each value, zero from avail on
        for (_, avail, shift, bits), vals, col in zip(cols, values, cols):
            assert cr.column_scalars(cells, col, ln) == [vals[i] & ((1 << bits) - 1) if i < avail else 0
                                                         for i in range(ln)]
        if ln <= 64:  # column 0 point by point (the same cells for both curves' calls)
            if (cv, ln) not in _naive_cache:
                pts = mr.known_bases(form, ln)[1]
                _naive_cache[cv, ln] = mr.bitwise_msm(cv, cr.column_scalars(cells, cols[0], ln), pts)
            assert got[0] == _naive_cache[cv, ln], (form, ln)


def _recoding_cells(c):
    n = cr.windows(32, c)
    half = 1 << (c - 1)
    out = [ALL,                                                   # every digit 2^c - 1: the carry runs to the top
           sum(half << (w * c) for w in range(n)) & ALL,          # every digit exactly 2^(c-1): kept
           sum((half + 1) << (w * c) for w in range(n)) & ALL, 0, 1]
    for edge in range(0, 32 + c, c):
        for k in (edge - 1, edge, edge + 1):
            if 0 < k <= 32:
                out.append((1 << k) - 1)
    return out


@pytest.mark.parametrize("c", [1, 2, 5, 8, 13, 16])
def test_forced_window_widths_and_carries(diag_engine, c):
    from b2f import _lib

    assert "B2F_DIAG_MSM_PLAN" not in os.environ
    try:
        os.environ["B2F_DIAG_MSM_PLAN"] = str(c)
        rng = random.Random(200 + c)
        sp = _recoding_cells(c)
        ln = len(sp) + 40
        col = sp + [rng.randrange(1 << 32) for _ in range(40)]
        cells = np.array(col + col[::-1], dtype=np.uint32)
        cols = [(0, ln, 0, 32), (ln, ln, 0, 32), (0, ln, 3, 17), (0, ln, 0, 16), (ln, ln, 16, 16), (0, ln, c % 32, 1)]
        plan = _lib.msm_cells_plan(cols, ln, diag=True)
        assert plan["window_bits"] == c and plan["digits"] == cr.digit_count(cols, ln, c)
        for form in (1, 3):
            bs, d_b = _bases(form, ln)
            assert _call(diag_engine, form, cells, cols, ln, d_b) == _expect(form, cells, cols, ln, bs), (c, form)
    finally:
        os.environ.pop("B2F_DIAG_MSM_PLAN", None)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_tail(engine, form):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(300 + form)
    ln = 50
    cells = np.array([rng.randrange(1 << 32) for _ in range(3 * ln)], dtype=np.uint32)
    cols = [(0, ln, 0, 32), (ln, ln, 0, 16), (2 * ln, ln - 7, 5, 9)]
    bs, d_b = _bases(form, ln + 64)
    plain = _call(engine, form, cells, cols, ln, d_b)
    assert plain == _expect(form, cells, cols, ln, bs)  # tail_rows = 0: the cells-only sum
    for rows in (1, 6, 64):
        tail = [[rng.randrange(r) for _ in range(rows)] for _ in cols]
        tail[0][0], tail[1][rows - 1], tail[2][rows // 2] = 0, r - 1, 1
        if rows > 1:
            tail[1][0] = 1
            tail[2][rows - 1] = 0
        got = _call(engine, form, cells, cols, ln, d_b, tail=tail)
        assert got == _expect(form, cells, cols, ln, bs, tail=tail), (form, rows)
        assert got != plain
        zero = _call(engine, form, cells, cols, ln, d_b, tail=[[0] * rows for _ in cols])
        assert zero == plain, "an all-zero tail adds nothing"
    # len = 1 with a tail; a column with no cells at all is its tail alone
    tail = [[rng.randrange(r) for _ in range(6)] for _ in range(2)]
    cols1 = [(3, 1, 0, 32), (4, 0, 0, 32)]
    got = _call(engine, form, cells, cols1, 1, d_b, tail=tail)
    assert got == _expect(form, cells, cols1, 1, bs, tail=tail)
    assert got[1] == mr.expected_msm(form, tail[1], bs[1:7])
    if form in (1, 3):  # the same sums point by point
        pts = mr.known_bases(form, 7)[1]
        assert got[0] == mr.bitwise_msm(cv, [int(cells[3])] + tail[0], pts)


@pytest.mark.parametrize("form", [1, 3])
def test_real_trace_three_circuits_against_the_exported_block(engine, form):
    import torch

    import b2f
    from b2f import synth

    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(400 + form)
    x = synth.batch(5, rounds_mix=[0, 1, 12], seed=77)
    x["rounds"][:3] = [12, 0, 1]
    batch = b2f.DeviceBatch(x, device="cuda:0")
    total = batch.total_rows
    assert 3000 < total < 30000
    batch.fill_evaluate(engine)
    usable, tail_rows = 3000, 6
    begins = [0, 117, total - 1000]  # mid-instance; the last runs 2,000 rows past the trace
    bs, d_b = _bases(form, usable + tail_rows)
    tail = [[rng.randrange(r) for _ in range(tail_rows)] for _ in range(30)]
    d_tail = _tail_block(form, tail)
    got = batch.commit_advice(engine, begins, usable, d_b, tail=d_tail, form=form)
    one = batch.commit_advice(engine, begins[1], usable, d_b, tail=d_tail[10:20].contiguous(), form=form)
    fixed = batch.commit_fixed(engine, begins[1], usable, d_b, form=form)
    fixed_past = batch.commit_fixed(engine, begins[2], usable, d_b, form=form)
    # the parent path on the device: export, write the tail rows into the block, b2f_msm_dev
    for c, begin in enumerate(begins):
        block = torch.zeros((10, usable + tail_rows, 4), dtype=torch.int64, device="cuda:0")
        batch.export_fp(engine, begin, min(usable, total - begin), form=form, out=block)
        block[:, usable:] = d_tail[10 * c:10 * c + 10]
        assert torch.equal(engine.msm(block, d_b, form=form), got[10 * c:10 * c + 10]), ("circuit", c)
    assert torch.equal(one, got[10:20])
    for begin, pts in ((begins[1], fixed), (begins[2], fixed_past)):
        block = torch.zeros((17, usable, 4), dtype=torch.int64, device="cuda:0")
        batch.export_fixed_fp(engine, begin, min(usable, total - begin), form=form, out=block)
        assert torch.equal(engine.msm(block, d_b, form=form), pts), ("fixed", begin)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    # and the big integers, from the host copy of the trace
    adv, fx = batch.host_trace()
    want = []
    for c, begin in enumerate(begins):
        for h in range(10):
            a = cr.HALO2_INDEX.index(h)
            col = [int(v) for v in adv[a, begin:begin + usable]]
            want.append(mr.expected_msm(form, col + [0] * (usable - len(col)) + tail[10 * c + h], bs))
    assert mr.unpack_points(cv, got.cpu().numpy()) == want
    begin = begins[1]
    q = [int(v) for v in fx[begin:begin + usable]]
    want = [mr.expected_msm(form, [(v >> c) & 1 for v in q], bs) for c in range(16)]
    want.append(mr.expected_msm(form, [v >> 16 for v in q], bs))
    assert mr.unpack_points(cv, fixed.cpu().numpy()) == want


def _advice_column(engine, ln):
    """A real advice column of the chip (a_1, the dense 16-bit limbs of the spread lookups)."""
    import torch

    import b2f
    from b2f import synth

    batch = b2f.DeviceBatch(synth.batch(14, rounds_mix=[12]), device="cuda:0")
    assert batch.used_rows >= ln
    batch.fill(engine)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    col = batch.host_trace()[0][1, :ln].astype(np.uint32)
    assert len(set(col.tolist())) > 1
    return col


@pytest.mark.parametrize("form", [1, 3])
def test_cell_distributions(engine, form):
    cv = mr.curve_of_form(form)
    ln = (1 << 16) + 3
    bs, d_b = _bases(form, BIG, incremental=True)
    bs = bs[:ln]
    rows = [np.zeros(ln, dtype=np.uint32), np.ones(ln, dtype=np.uint32), np.full(ln, ALL, dtype=np.uint32)]
    for at in (0, ln // 2, ln - 1):
        one = np.zeros(ln, dtype=np.uint32)
        one[at] = 0x9e3779b9
        rows.append(one)
    rows.append(_advice_column(engine, ln))
    cells = np.concatenate(rows)
    cols = [(j * ln, ln, 0, 32) for j in range(len(rows))]
    got = _call(engine, form, cells, cols, ln, d_b)
    assert got == _expect(form, cells, cols, ln, bs)
    assert got[0] is None
    assert got[1] == mr.gen_mul(cv, sum(bs) % mr.ORDER[cv])  # the all-ones column is the sum of the bases
    assert got[3] == mr.gen_mul(cv, 0x9e3779b9 * bs[0] % mr.ORDER[cv])


@pytest.mark.parametrize("form", [1, 3])
def test_size_and_batching(engine, diag_engine, form):
    from b2f import _lib

    rng = np.random.default_rng(500 + form)
    bs, d_b = _bases(form, BIG, incremental=True)
    cells = rng.integers(0, 1 << 32, 10 * BIG, dtype=np.uint64).astype(np.uint32)
    cols = [(j * BIG, BIG, 0, 32) for j in range(10)]
    assert _call(engine, form, cells, cols, BIG, d_b) == _expect(form, cells, cols, BIG, bs)
    # 5 columns in one call = five single-column calls (and the reference); mixed widths
    ln = 3001
    mixed = [(j * BIG + j, ln - (j == 2), s, b) for j, (s, b) in enumerate(SHAPES + [(0, 32)])]
    want = _expect(form, cells, mixed, ln, bs[:ln])
    assert _call(engine, form, cells, mixed[:5], ln, d_b) == want[:5]
    assert [_call(engine, form, cells, [c], ln, d_b)[0] for c in mixed[:5]] == want[:5]
    assert "B2F_DIAG_MSM_PLAN" not in os.environ
    try:
        c = _lib.msm_cells_plan(mixed[:5], ln, form=form)["window_bits"]
        os.environ["B2F_DIAG_MSM_PLAN"] = "%d,2" % c
        assert _call(diag_engine, form, cells, mixed[:5], ln, d_b) == want[:5]
        assert _call(diag_engine, form, cells, mixed, ln, d_b) == want
        # c = 1: 33 digits a cell, 17.3 M for this column, more than a pass holds: two row chunks
        os.environ["B2F_DIAG_MSM_PLAN"] = "1"
        ln = (1 << 19) + 3
        col = [(5, ln, 0, 32)]
        assert _lib.msm_cells_plan(col, ln, diag=True)["digits"] == 33 * ln > 1 << 24
        bs2, d_b2 = _bases(form, ln)
        assert _call(diag_engine, form, cells, col, ln, d_b2) == _expect(form, cells, col, ln, bs2)
    finally:
        os.environ.pop("B2F_DIAG_MSM_PLAN", None)


def test_scratch_shared_with_the_full_width_calls():
    import torch

    import b2f

    form, cv = 1, 0
    r = mr.ORDER[cv]
    rng = random.Random(600)
    eng = b2f.Engine(0)
    try:
        bs, d_b = _bases(form, 20000)
        cells = np.array([rng.randrange(1 << 32) for _ in range(4 * 20000)], dtype=np.uint32)
        big = [(j * 20000, 20000, 0, 32) for j in range(4)]
        assert _call(eng, form, cells, big, 20000, d_b) == _expect(form, cells, big, 20000, bs)
        sc = [[rng.randrange(r) for _ in range(5)]]
        out = eng.msm(_dev(np.stack([mr.pack_scalars(form, c) for c in sc])), d_b, form=form)
        assert mr.unpack_points(cv, out.cpu().numpy()) == [mr.expected_msm(form, sc[0], bs)]
        n = 1 << 12  # a round longer than the direct kernel takes: the two-column pass in the same scratch
        assert n > b2f._lib.ipa_direct_max_len()
        p, b = [rng.randrange(r) for _ in range(n)], [rng.randrange(r) for _ in range(n)]
        lr, vals = eng.ipa_round(_dev(mr.pack_scalars(form, p)), _dev(mr.pack_scalars(form, b)), d_b, len=n, form=form)
        eng.sync(torch.cuda.current_stream().cuda_stream)
        assert mr.unpack_points(cv, lr.cpu().numpy()) == ir.points_of(cv, ir.round_known(cv, p, bs[:n]))
        assert np.array_equal(vals.cpu().numpy().view(np.uint64).reshape(-1, 4), mr.pack_scalars(form, ir.values(cv, p, b)))
        small = [(7, 5, 0, 32), (1, 3, 4, 8)]
        tail = [[rng.randrange(r)] for _ in small]
        assert _call(eng, form, cells, small, 5, d_b, tail=tail) == _expect(form, cells, small, 5, bs, tail=tail)
        cells2 = cells[::-1].copy()
        big2 = [(j * 19999 + 1, 19999, 0, 32) for j in range(4)]
        assert _call(eng, form, cells2, big2, 19999, d_b) == _expect(form, cells2, big2, 19999, bs)
    finally:
        eng.close()


def test_refused_arguments_and_timing(engine):
    import torch

    from b2f import B2FError

    form, cv, ln, n_cells, rows = 1, 0, 40, 100, 6
    rng = random.Random(700)
    bs, d_b = _bases(form, ln + rows)
    cells = np.array([rng.randrange(1 << 32) for _ in range(n_cells)], dtype=np.uint32)
    cols = [(3, ln, 0, 32), (50, ln + 9, 4, 12)]
    tail = [[rng.randrange(mr.ORDER[cv]) for _ in range(rows)] for _ in cols]
    want = _expect(form, cells, cols, ln, bs, tail=tail)
    d_cells, d_tail = _dev_cells(cells), _tail_block(form, tail)
    d_out = torch.zeros((2, 8), dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    C, T, Bp, O, nb = d_cells.data_ptr(), d_tail.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), ln + rows

    def call(cells=C, n_cells=n_cells, cols=cols, ln=ln, tail=T, rows=rows, bases=Bp, n_bases=nb, form=form, out=O):
        engine.msm_cells_dev(cells, n_cells, cols, ln, tail, rows, bases, n_bases, form, out, s)

    def good():
        d_out.zero_()
        call()
        engine.sync(s)
        assert mr.unpack_points(cv, d_out.cpu().numpy()) == want

    good()
    col = lambda *d: [cols[0], d]  # noqa: E731
    refused = [
        (ERR_ARG, dict(cells=0)), (ERR_ARG, dict(bases=0)), (ERR_ARG, dict(out=0)),
        (ERR_ARG, dict(cells=C + 4)), (ERR_ARG, dict(bases=Bp + 8)), (ERR_ARG, dict(out=O + 8)),
        (ERR_ARG, dict(tail=T + 8)),
        (ERR_ARG, dict(form=4)), (ERR_ARG, dict(ln=0)), (ERR_ARG, dict(ln=(1 << 28) + 1, n_bases=1 << 30)),
        (ERR_ARG, dict(cols=[])), (ERR_ARG, dict(cols=[(0, 1, 0, 32)] * 4097)),
        (ERR_ARG, dict(rows=65, n_bases=1 << 20)), (ERR_ARG, dict(rows=0)), (ERR_ARG, dict(tail=0)),
        (ERR_ARG, dict(cols=col(0, ln, 0, 0))), (ERR_ARG, dict(cols=col(0, ln, 0, 33))),
        (ERR_ARG, dict(cols=col(0, ln, 1, 32))), (ERR_ARG, dict(cols=col(0, ln, 32, 1))),
        (ERR_ARG, dict(out=C)), (ERR_ARG, dict(out=C + 4 * n_cells - 16)),       # the output on the cells
        (ERR_ARG, dict(out=Bp + 64 * (nb - 1))), (ERR_ARG, dict(out=T + 64)),   # ... on a base, on the tail
        (ERR_ROWS, dict(cols=col(n_cells - ln + 1, ln, 0, 32))),                 # one cell past the end
        (ERR_ROWS, dict(cols=col(n_cells - 5, 6, 0, 32))), (ERR_ROWS, dict(cols=col(n_cells + 1, 0, 0, 32))),
        (ERR_ROWS, dict(cols=col(1 << 63, 1 << 63, 0, 32))),
        (ERR_ROWS, dict(n_bases=nb - 1)),                                        # len + tail_rows > n_bases
    ]
    for code, kw in refused:
        with pytest.raises(B2FError) as e:
            call(**kw)
        assert e.value.code == code, kw
        good()
    # what is allowed at the edges: the last cell, an avail past the cells that len cuts off
    call(cols=col(n_cells - ln, ln, 0, 32))
    call(cols=col(n_cells - ln, 1 << 40, 0, 32))
    call(cols=col(n_cells, 0, 0, 32))
    good()
    engine.set_timing(True)
    call()
    times = engine.kernel_times()
    engine.set_timing(False)
    assert times["quotient"][1] == 1 and times["quotient"][0] > 0
    assert all(v[1] == 0 for k, v in times.items() if k != "quotient")
