"""The host side of b2f_msm_cells_dev without a device: the recoding model of tests/cells_ref.py
against itself (the digits sum back, their size, their count), b2f_msm_cells_plan through ctypes
against the model, the two descriptor functions against their formulas, and the header, the Rust
binding and the ctypes table against each other."""
import ctypes
import random

import pytest

import cells_ref as cr

ERR_ARG = 1
CAP_ENTRIES, CAP_BUCKETS = 1 << 24, 1 << 20  # a pass: digits, buckets (128 bytes each)


def _cells_for(bits, c, rng):
    """Values below 2^bits: 0, 1, all ones, every digit at and around 2^(c-1) and at 2^c - 1, single
    bits and 2^k - 1 around every window edge, and 1,000 random ones."""
    top = (1 << bits) - 1
    n = cr.windows(bits, c)
    out = {0, 1, top}
    for d in ((1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1):
        out.add(sum(d << (w * c) for w in range(n)) & top)
        for w in range(n):
            out.add((d << (w * c)) & top)
    for edge in range(0, bits + c, c):
        for k in (edge - 1, edge, edge + 1):
            if 0 <= k <= bits:
                out.add((1 << k) - 1)
                out.add((1 << k) & top)
    return sorted(out) + [rng.randrange(top + 1) for _ in range(1000)]


@pytest.mark.parametrize("c", range(1, 17))
def test_recoding_model(c):
    rng = random.Random(900 + c)
    half = 1 << (c - 1)
    for bits in range(1, 33):
        n = cr.windows(bits, c)
        assert n == (bits + 1 + c - 1) // c and n * c >= bits + 1 > (n - 1) * c
        for v in _cells_for(bits, c, rng):
            d = cr.recode(v, bits, c)
            assert len(d) == n
            assert sum(x << (w * c) for w, x in enumerate(d)) == v, (c, bits, v)
            assert all(-half <= x <= half for x in d), (c, bits, v)
        # the field of a cell: a few shifts, the bits around it all ones or all zeros
        for shift in sorted({0, (32 - bits) // 2, 32 - bits}):
            v = rng.randrange(1 << bits)
            outside = 0xffffffff ^ (((1 << bits) - 1) << shift)
            assert cr.scalar(v << shift, shift, bits) == v == cr.scalar((v << shift) | outside, shift, bits)
    # a digit of exactly 2^(c-1) is kept, one above it borrows
    assert cr.recode(half, c, c)[0] == half
    if c > 1:
        assert cr.recode(half + 1, c, c)[:2] == [half + 1 - (1 << c), 1]


MIXED = [(0, 1 << 30, 0, 32), (5, 1 << 30, 0, 16), (9, 7, 16, 16), (2, 1 << 30, 0, 1), (3, 0, 7, 1), (1, 9, 3, 17)]


def test_plan_digits_match_the_model():
    from b2f import _lib

    for ln in (1, 2, 63, 1000, (1 << 16) + 3, 1 << 17, 1 << 20, 1 << 28):
        for cols in ([MIXED[0]], [MIXED[1]], [MIXED[3]], MIXED, MIXED * 100, cr.fixed_columns(1 << 20, 0, 1 << 20)):
            p = _lib.msm_cells_plan(cols, ln)
            c = p["window_bits"]
            assert 1 <= c <= 16
            assert p["digits"] == cr.digit_count(cols, ln, c), (ln, len(cols))
            assert p == _lib.msm_cells_plan(cols, ln, tail_rows=64, form=3)  # neither changes the plan
    # what the cell path is for: a 32-bit cell is 4 digits at 2^17 rows and 3 at 2^20 (a field
    # element: 26 and 24), a 16-bit limb 2, a bit 1
    for ln, wide in ((1 << 17, 4), (1 << 20, 3)):
        assert _lib.msm_cells_plan([MIXED[0]], ln)["digits"] == wide * ln
        assert _lib.msm_cells_plan([MIXED[1]], ln)["digits"] == 2 * ln
        assert _lib.msm_cells_plan([MIXED[3]], ln)["digits"] == ln


def _pass_capacity_bytes(n_cols, sum_w):
    """The scratch of one full pass (2^24 digits, 2^20 buckets) plus the per-column blocks: what no
    call may exceed however long or wide it is."""
    e = CAP_ENTRIES
    n1 = 2 * (e // 32)
    n2 = 2 * -(-n1 // 32)
    sort = 9 * e + (1 << 20)
    per_col = (128 + 128 + 32) * n_cols
    return 16 * e + sort + 132 * (n1 + n2) + 128 * CAP_BUCKETS + 128 * min(sum_w, CAP_BUCKETS) + per_col + 16 * 256


def test_plan_scratch_is_bounded_by_a_pass_and_never_shrinks():
    from b2f import _lib

    wide = [MIXED[0]] * 4096
    big = _lib.msm_cells_plan(wide, 1 << 28)
    sum_w = big["digits"] >> 28
    assert big["digits"] > 1000 * CAP_ENTRIES  # far more than a pass holds: it is cut into passes
    assert big["scratch_bytes"] <= _pass_capacity_bytes(4096, sum_w)
    # growing len at fixed columns, growing columns at fixed len
    lens = sorted({min(max(1, (1 << k) + d), 1 << 28) for k in range(29) for d in (-1, 0, 1)})
    for cols in ([MIXED[0]], MIXED, [MIXED[0]] * 10):
        last = 0
        for ln in lens:
            sb = _lib.msm_cells_plan(cols, ln)["scratch_bytes"]
            assert sb >= last, (len(cols), ln)
            last = sb
    for ln in (1, 300, 1 << 17, 1 << 24):
        last = 0
        for n in (1, 2, 3, 10, 11, 64, 640, 4096):
            sb = _lib.msm_cells_plan((MIXED * 700)[:n], ln)["scratch_bytes"]
            assert sb >= last, (ln, n)
            last = sb


def test_plan_refuses_what_the_call_refuses():
    from b2f import B2FError, _lib

    good = [MIXED[0]]
    assert _lib.msm_cells_plan(good, 40)["digits"] > 0
    refused = [
        dict(cols=good, len_=0), dict(cols=good, len_=(1 << 28) + 1), dict(cols=[], len_=40),
        dict(cols=good * 4097, len_=40), dict(cols=good, len_=40, tail_rows=65), dict(cols=good, len_=40, form=4),
        dict(cols=[(0, 40, 0, 0)], len_=40), dict(cols=[(0, 40, 0, 33)], len_=40),
        dict(cols=[(0, 40, 1, 32)], len_=40), dict(cols=[(0, 40, 31, 2)], len_=40),
        dict(cols=[(0, 40, 32, 1)], len_=40), dict(cols=good + [(0, 40, 17, 16)], len_=40),
    ]
    for kw in refused:
        with pytest.raises(B2FError) as e:
            _lib.msm_cells_plan(**kw)
        assert e.value.code == ERR_ARG, kw
    lib = _lib.load()
    assert lib.b2f_msm_cells_plan(None, 1, 40, 0, 1, None, None, None) == ERR_ARG
    assert lib.b2f_msm_cells_plan(_lib.cell_columns(good), 1, 40, 0, 1, None, None, None) == 0  # outputs may be null
    assert _lib.msm_cells_plan(good * 4096, 1 << 28, tail_rows=64)["digits"] > 0  # the limits themselves


def test_descriptor_functions_match_their_formulas():
    import b2f
    from b2f import _lib

    cases = [(4096, 0, 4096), (4096, 100, 1000), (4096, 4000, 1000),  # straddles the end: 96 rows left
             (4096, 4095, 7), (4096, 4096, 1000), (4096, 9000, 1000),  # at and past the end: nothing left
             (1 << 20, 12345, 1 << 17), (8, 3, 1 << 28)]
    for total, begin, usable in cases:
        adv = b2f.advice_cell_columns(total, begin, usable)
        assert adv == cr.advice_columns(total, begin, usable), (total, begin, usable)
        left = max(0, total - begin)
        for i in range(10):
            assert adv[b2f.halo2_column_index(i)] == (i * total + begin, min(usable, left), 0, 32)
        fx = b2f.fixed_cell_columns(total, begin, usable)
        assert fx == cr.fixed_columns(total, begin, usable)
        assert fx[16] == (begin, min(usable, left), 16, 16) and fx[5] == (begin, min(usable, left), 5, 1)
    assert cr.advice_columns(4096, 4000, 1000)[0][1] == 96 and cr.advice_columns(4096, 4096, 5)[0][1] == 0
    lib = _lib.load()
    buf = (_lib.CellColumn * 17)()
    for total, usable in ((4098, 100), (4096, 0), (3, 1)):
        assert lib.b2f_advice_cell_columns(total, 0, usable, buf) == 0
        assert lib.b2f_fixed_cell_columns(total, 0, usable, buf) == 0
        for fn in (b2f.advice_cell_columns, b2f.fixed_cell_columns):
            with pytest.raises(b2f.B2FError):
                fn(total, 0, usable)
    assert all(d.bits == 0 and d.offset == 0 for d in buf), "a refused call wrote descriptors"
    assert lib.b2f_advice_cell_columns(4096, 0, 10, None) == 0
    assert lib.b2f_advice_cell_columns(4096, 0, 10, buf) == 10 and lib.b2f_fixed_cell_columns(4096, 0, 10, buf) == 17


NAMES = ["b2f_msm_cells_dev", "b2f_msm_cells_plan", "b2f_advice_cell_columns", "b2f_fixed_cell_columns"]


def test_header_binding_and_ctypes_agree():
    import test_integration_binding as tib
    from b2f import _lib

    hdr, (rust, links) = tib.header_functions(), tib.rust_externs()
    ctab = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    val = {"u64": ctypes.c_uint64, "u32": ctypes.c_uint32, "i32": ctypes.c_int}
    for name in NAMES:
        assert hdr[name] == rust[name] and links[name] == "b2f", name
        ret, args = hdr[name]
        res, cargs = ctab[name]
        assert res is val[ret[1]], name
        assert cargs == [ctypes.c_void_p if kind != "val" else val[base] for kind, base in args], name
    assert len(hdr["b2f_msm_cells_dev"][1]) == 13 and len(hdr["b2f_msm_cells_plan"][1]) == 8
    # the struct: header, Rust and ctypes field for field, 24 bytes
    fields = tib.header_structs()["b2f_cell_column"]
    assert fields == tib.rust_structs()["B2fCellColumn"] == [("offset", "u64", 1), ("avail", "u64", 1),
                                                             ("shift", "u32", 1), ("bits", "u32", 1)]
    assert [f[0] for f in _lib.CellColumn._fields_] == [f[0] for f in fields]
    assert ctypes.sizeof(_lib.CellColumn) == 24 == sum(tib.RUST_SIZES[t] * n for _, t, n in fields)
    assert "size_of::<B2fCellColumn>() == 24" in open(tib.DOC).read()
    for lib in (_lib.load(), _lib.load(diag=True)):
        for name in NAMES:
            assert hasattr(lib, name), name
