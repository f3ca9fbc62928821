"""b2f_ntt_columns_dev against the big-integer reference (tests/ntt_ref.py, which
tests/test_ntt_ref.py pins to the O(n^2) definition).

  1  k = 1..6, every form, both directions, shift 1 and random, against the O(n^2) definition;
     padded strides, rows >= n of the output untouched;
  2  every k from 7 to 16, every row against the reference;
  3  zero padding (in_len < n) with a cube-root-of-unity shift, garbage past in_len;
  4  each pass plan at scale. One pass: k <= 10; two passes: k = 11..16; three passes:
     k = 17..24; four: k = 25..28. The smallest and the largest k of each plan up to k = 25: a
     sparse input against its six-term direct sum, and inverse(forward(x)) == x on a dense input.
     Four passes run at k = 25 (1 GiB per column); k = 26..28 run the same code with wider digits
     and stay unrun here (2 to 8 GiB per column): no 32-bit quantity in the kernel grows past
     2^28 (row indices, digit values, twiddle exponents after their mask), and the exponent
     products are formed in 64 bits. tests/test_gpu_ntt_plans.py runs three- and four-pass plans
     at k = 11..16 against the reference on every row;
  5  65,537 columns at k = 1; 130 columns at k = 10 against single-column calls; three columns
     with padded strides at k = 11 and k = 17 (two and three passes), in_len = n / 4;
  6  the permutation z column of a k = 10 circuit: to coefficients and to an extended coset;
  7  the table cache: domains alternate, another generator of the same domain;
  8  every argument error of the header, the primitive-root check at sync;
  9  one call is one `ntt` timed region.

Needs an MI355X (`-m gpu`)."""
import ctypes

import numpy as np
import pytest

import ntt_ref as nr

from conftest import random_inputs

pytestmark = pytest.mark.gpu

FWD, INV = 0, 1
ERR_ARG, ERR_ROWS, ERR_FIELD = 1, 3, 7


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _omega(form, k):
    from b2f import field

    return field.omega(field.of_form(form), k)


def _cube_root(form):
    from b2f import field

    f, p = field.of_form(form), nr.modulus(form)
    z = pow(field.GENERATOR[f], (p - 1) // 3, p)
    assert z != 1 and pow(z, 3, p) == 1
    return z


def _shift(rng, p):
    return 2 + nr.random_elements(rng, 1, p - 2)[0]


def _pattern(shape):
    """A recognisable fill for output buffers."""
    return np.full(shape, 0xA5A5A5A5DEADBEEF, dtype=np.uint64)


def _run(engine, x, in_len, k, direction, shift, form, omega=None, out_rows=None):
    """x: uint64 [cols, in_rows, 4] host limbs. Returns the host output [cols, out_rows, 4]
    (out_rows > n: rows past n keep the pattern)."""
    n = 1 << k
    out_rows = n if out_rows is None else out_rows
    d_in = _dev(x)
    d_out = _dev(_pattern((x.shape[0], out_rows, 4)))
    engine.ntt_columns_dev(d_in.data_ptr(), x.shape[1], in_len, x.shape[0], k,
                           _omega(form, k) if omega is None else omega, shift, direction, form,
                           d_out.data_ptr(), out_rows, _stream())
    engine.sync(_stream())
    return _host(d_out)


def _expect(vals, in_len, k, direction, shift, form, omega=None):
    p = nr.modulus(form)
    w = _omega(form, k) if omega is None else omega
    if direction == FWD:
        return nr.forward(vals[:in_len], k, w, shift, p)
    return nr.inverse(list(vals[:in_len]) + [0] * ((1 << k) - in_len), k, w, shift, p)


def _first_diff(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return int(bad[0]) if len(bad) else None


# ---------------------------------------------------------------------------------------------
# 1. the definition, tiny


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_definition_tiny(engine, form):
    p = nr.modulus(form)
    rng = np.random.default_rng(40 + form)
    for k in range(1, 7):
        n = 1 << k
        w = _omega(form, k)
        for direction in (FWD, INV):
            for shift in (1, _shift(rng, p)):
                in_len = n if direction == INV else max(1, n - 1)
                in_rows, out_rows = n + 3, n + 5
                cols = [nr.random_elements(rng, in_rows, p) for _ in range(3)]
                x = np.stack([nr.pack(c, form) for c in cols])
                got = _run(engine, x, in_len, k, direction, shift, form, out_rows=out_rows)
                for c in range(3):
                    if direction == FWD:
                        want = nr.forward_def(cols[c][:in_len], k, w, shift, p)
                    else:
                        want = nr.inverse_def(cols[c][:n], k, w, shift, p)
                    assert _first_diff(got[c, :n], nr.pack(want, form)) is None, (k, direction, shift, c)
                    assert (got[c, n:] == _pattern((out_rows - n, 4))).all(), (k, direction, c)


# ---------------------------------------------------------------------------------------------
# 2. every k from 7 to 16


@pytest.mark.parametrize("k", list(range(7, 17)))
def test_every_row_k7_to_k16(engine, k):
    form = k % 4
    p = nr.modulus(form)
    n = 1 << k
    rng = np.random.default_rng(200 + k)
    cols = [nr.random_elements(rng, n, p)]
    if k <= 14:
        cols.append([(0, 1, p - 1)[v] for v in rng.integers(0, 3, n)])
    else:  # one column: the special values ride in the dense one
        cols[0][:3] = [0, 1, p - 1]
        cols[0][n - 1] = p - 1
    x = np.stack([nr.pack(c, form) for c in cols])
    shift = _shift(rng, p)
    for direction in (FWD, INV):
        got = _run(engine, x, n, k, direction, shift, form)
        for c, vals in enumerate(cols):
            want = nr.pack(_expect(vals, n, k, direction, shift, form), form)
            assert _first_diff(got[c], want) is None, (direction, c, _first_diff(got[c], want))


# ---------------------------------------------------------------------------------------------
# 3. zero padding


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("in_len", [1, 1 << 10, (1 << 12) - 1])
def test_zero_padding(engine, form, in_len):
    k, n = 12, 1 << 12
    p = nr.modulus(form)
    zeta = _cube_root(form)
    rng = np.random.default_rng(300 + in_len % 97 + form)
    vals = nr.random_elements(rng, n, p)  # rows >= in_len: non-zero garbage that must not count
    assert all(v != 0 for v in vals[in_len:])
    x = nr.pack(vals, form)[None]
    got = _run(engine, x, in_len, k, FWD, zeta, form)
    want = nr.pack(nr.forward(vals[:in_len], k, _omega(form, k), zeta, p), form)
    assert _first_diff(got[0], want) is None
    # the same rows in a buffer that ends at in_len: nothing past it is read
    got2 = _run(engine, x[:, :in_len], in_len, k, FWD, zeta, form)
    assert (got2 == got).all()


# ---------------------------------------------------------------------------------------------
# 4. each pass plan at scale

T = 10  # log2 of the tile


def _random_device(n_cols, rows, seed):
    """Dense random elements < 2^253 (below both moduli, a valid element in any form)."""
    import torch

    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    shape = (n_cols, rows, 4)
    x = torch.randint(0, 2**32, shape, dtype=torch.int64, device="cuda:0", generator=g) << 32
    x |= torch.randint(0, 2**32, shape, dtype=torch.int64, device="cuda:0", generator=g)
    x[:, :, 3] &= (1 << 61) - 1
    return x


@pytest.mark.parametrize("k", [1, 10, 11, 16, 17, 23, 24, 25])
def test_pass_plans(engine, k):
    import torch

    form = 1 if k % 2 else 3
    p = nr.modulus(form)
    n = 1 << k
    w = _omega(form, k)
    rng = np.random.default_rng(400 + k)
    shift = _shift(rng, p)
    # (a) sparse input against its direct sum
    pos = sorted({j for j in (0, 1, (1 << T) - 1, 1 << T, n // 2 + 3, n - 1) if j < n})
    coef = nr.random_elements(rng, len(pos), p)
    x = torch.zeros((1, n, 4), dtype=torch.int64, device="cuda:0")
    x[0, torch.tensor(pos, device="cuda:0")] = _dev(nr.pack(coef, form))
    out = engine.ntt_columns(x, k, shift=shift, form=form)
    engine.sync(_stream())
    rows = sorted({0, 1, n - 1} | set(int(r) for r in rng.integers(0, n, 4096)))
    got = _host(out[0, torch.tensor(rows, device="cuda:0")])
    want = []
    for i in rows:
        pt = shift * pow(w, i, p) % p
        want.append(sum(c * pow(pt, j, p) for j, c in zip(pos, coef)) % p)
    bad = _first_diff(got, nr.pack(want, form))
    assert bad is None, "row %d" % rows[bad]
    del x, out
    # (b) dense input: the inverse undoes the forward bit for bit
    x = _random_device(1, n, 4000 + k)
    y = engine.ntt_columns(x, k, shift=shift, form=form)
    back = engine.ntt_columns(y, k, inverse=True, shift=shift, form=form)
    engine.sync(_stream())
    assert not torch.equal(y, x)
    assert torch.equal(back, x)


# ---------------------------------------------------------------------------------------------
# 5. many columns


def test_more_columns_than_a_grid_dimension(engine):
    form, k, n_cols = 0, 1, 65537
    p = nr.modulus(form)
    rng = np.random.default_rng(50)
    shift = _shift(rng, p)
    vals = nr.random_elements(rng, 2 * n_cols, p)
    x = nr.pack(vals, form).reshape(n_cols, 2, 4)
    got = _run(engine, x, 2, k, FWD, shift, form)
    want = []
    for c in range(n_cols):
        a, b = vals[2 * c], vals[2 * c + 1] * shift % p
        want += [(a + b) % p, (a - b) % p]  # omega = -1
    assert _first_diff(got.reshape(-1, 4), nr.pack(want, form)) is None


def test_columns_equal_single_column_calls(engine):
    import torch

    form, k, n_cols = 3, 10, 130
    p = nr.modulus(form)
    n = 1 << k
    rng = np.random.default_rng(51)
    shift = _shift(rng, p)
    x = _random_device(n_cols, n, 5100)
    for inverse in (False, True):
        out = engine.ntt_columns(x, k, inverse=inverse, shift=shift, form=form)
        single = torch.stack([engine.ntt_columns(x[c:c + 1], k, inverse=inverse, shift=shift, form=form)[0]
                              for c in range(n_cols)])
        engine.sync(_stream())
        assert torch.equal(out, single)
        hx, hout = _host(x), _host(out)
        for c in (0, 64, 129):
            vals = nr.unpack(hx[c], form)
            want = nr.pack(_expect(vals, n, k, INV if inverse else FWD, shift, form), form)
            assert _first_diff(hout[c], want) is None, (inverse, c)


@pytest.mark.parametrize("k", [11, 17])
def test_padded_strides_on_multi_pass_sizes(engine, k):
    """Several columns whose strides are not n, where every pass after the first works in place on
    the output: each column equals its own single-column call, rows past n are never written, and
    at k = 11 every row equals the reference."""
    import torch

    form = 1 if k == 11 else 2
    p = nr.modulus(form)
    n, n_cols = 1 << k, 3
    in_rows, out_rows = n + 3, n + 5
    rng = np.random.default_rng(520 + k)
    shift = _shift(rng, p)
    x = _random_device(n_cols, in_rows, 5200 + k)
    pat = _dev(_pattern((n_cols, out_rows, 4)))
    for inverse, in_len in ((False, n // 4), (True, n)):
        out = engine.ntt_columns(x, k, inverse=inverse, shift=shift, in_len=in_len, form=form, out=pat.clone())
        single = [engine.ntt_columns(x[c:c + 1], k, inverse=inverse, shift=shift, in_len=in_len, form=form,
                                     out=pat[:1].clone()) for c in range(n_cols)]
        engine.sync(_stream())
        assert torch.equal(out, torch.cat(single)), inverse
        assert torch.equal(out[:, n:], pat[:, n:]), inverse
        assert not torch.equal(out[0, :n], out[1, :n])
        if k == 11:
            hx, hout = _host(x), _host(out)
            for c in range(n_cols):
                vals = nr.unpack(hx[c], form)
                want = nr.pack(_expect(vals, in_len, k, INV if inverse else FWD, shift, form), form)
                assert _first_diff(hout[c, :n], want) is None, (inverse, c)


# ---------------------------------------------------------------------------------------------
# 6. the library's own columns


def test_permutation_z_to_coefficients_and_extended_coset(engine):
    import torch

    import b2f

    form, k, ke = 1, 10, 12
    p = nr.modulus(form)
    n, usable = 1 << k, (1 << k) - 6
    x = random_inputs(2, (0,), 61)
    x["rounds"] = np.asarray([1, 0], dtype=np.uint32)
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    rng = np.random.default_rng(60)
    beta, gamma = nr.random_elements(rng, 2, p)
    _, z = batch.permutation_columns(engine, k, usable, beta, gamma, form=form, sigma=False)
    z[:, usable + 1:] = _dev(nr.pack(nr.random_elements(rng, n - usable - 1, p), form))  # blinding rows
    engine.sync(_stream())
    zh = [nr.unpack(c, form) for c in _host(z)]
    assert zh[0][0] == 1 and zh[-1][usable] == 1
    coeff = engine.ntt_columns(z, k, inverse=True, form=form)
    zeta = _cube_root(form)
    ext = engine.ntt_columns(coeff, ke, shift=zeta, form=form)
    engine.sync(_stream())
    assert tuple(coeff.shape) == (z.shape[0], n, 4) and tuple(ext.shape) == (z.shape[0], 1 << ke, 4)
    w, we = _omega(form, k), _omega(form, ke)
    rows = [0, 1, usable, n - 1] + [int(r) for r in rng.integers(0, n, 12)]
    rows_e = [0, 1, (1 << ke) - 1] + [int(r) for r in rng.integers(0, 1 << ke, 13)]
    for s, col in enumerate(_host(coeff)):
        cs = nr.unpack(col, form)
        for i in rows:
            assert nr.horner(cs, pow(w, i, p), p) == zh[s][i], (s, i)
        got = nr.unpack(_host(ext[s, torch.tensor(rows_e, device="cuda:0")]), form)
        for i, g in zip(rows_e, got):
            assert nr.horner(cs, zeta * pow(we, i, p) % p, p) == g, (s, i)


# ---------------------------------------------------------------------------------------------
# 7. the table cache


def test_domains_alternate_and_another_generator(engine):
    rng = np.random.default_rng(70)
    fa, ka, fb, kb = 1, 10, 3, 12
    pa, pb = nr.modulus(fa), nr.modulus(fb)
    va, vb = nr.random_elements(rng, 1 << ka, pa), nr.random_elements(rng, 1 << kb, pb)
    xa, xb = nr.pack(va, fa)[None], nr.pack(vb, fb)[None]
    sa, sb = _shift(rng, pa), _shift(rng, pb)
    a1 = _run(engine, xa, 1 << ka, ka, FWD, sa, fa)
    b1 = _run(engine, xb, 1 << kb, kb, FWD, sb, fb)
    a2 = _run(engine, xa, 1 << ka, ka, FWD, sa, fa)
    assert (a1 == a2).all()
    assert _first_diff(a1[0], nr.pack(_expect(va, 1 << ka, ka, FWD, sa, fa), fa)) is None
    assert _first_diff(b1[0], nr.pack(_expect(vb, 1 << kb, kb, FWD, sb, fb), fb)) is None
    # omega^3 generates the same domain: its own tables, its own result
    w3 = pow(_omega(fa, ka), 3, pa)
    for direction in (FWD, INV):
        got = _run(engine, xa, 1 << ka, ka, direction, sa, fa, omega=w3)
        want = nr.pack(_expect(va, 1 << ka, ka, direction, sa, fa, omega=w3), fa)
        assert _first_diff(got[0], want) is None, direction
        assert (got != _run(engine, xa, 1 << ka, ka, direction, sa, fa)).any()
    # more domains than the cache holds, then the first again
    for k in range(1, 10):
        vals = va[:1 << k]
        got = _run(engine, nr.pack(vals, fa)[None], 1 << k, k, INV, sa, fa)
        assert _first_diff(got[0], nr.pack(_expect(vals, 1 << k, k, INV, sa, fa), fa)) is None, k
    assert (_run(engine, xa, 1 << ka, ka, FWD, sa, fa) == a1).all()


# ---------------------------------------------------------------------------------------------
# 8. errors


def _limbs4(v):
    return (ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])


def test_argument_errors_then_a_good_call(engine):
    import torch

    from b2f import B2FError

    form, k = 1, 8
    p = nr.modulus(form)
    n = 1 << k
    rng = np.random.default_rng(80)
    vals = nr.random_elements(rng, n, p)
    buf = torch.empty((4 * n + 1, 4), dtype=torch.int64, device="cuda:0")
    buf[:n] = _dev(nr.pack(vals, form))
    buf[n:] = 0x5A5A5A5A
    before = buf.clone()
    d_in, d_out = buf.data_ptr(), buf.data_ptr() + 32 * 2 * n
    w = _omega(form, k)
    good = dict(d_in=d_in, in_rows=n, in_len=n, n_cols=1, k=k, omega=w, shift=1, direction=FWD,
                form=form, d_out=d_out, out_rows=n)

    def call(**kw):
        a = dict(good, **kw)
        engine.ntt_columns_dev(a["d_in"], a["in_rows"], a["in_len"], a["n_cols"], a["k"], a["omega"],
                               a["shift"], a["direction"], a["form"], a["d_out"], a["out_rows"], _stream())

    table = [
        (ERR_ARG, dict(d_in=0)), (ERR_ARG, dict(d_out=0)),
        (ERR_ARG, dict(d_in=d_in + 8)), (ERR_ARG, dict(d_out=d_out + 8)),
        (ERR_ARG, dict(k=0)), (ERR_ARG, dict(k=29, out_rows=1 << 29)),
        (ERR_ARG, dict(n_cols=0)), (ERR_ARG, dict(direction=2)), (ERR_ARG, dict(form=4)),
        (ERR_ARG, dict(in_len=0)),
        (ERR_ARG, dict(omega=p)), (ERR_ARG, dict(shift=p)), (ERR_ARG, dict(omega=2**256 - 1)),
        (ERR_ARG, dict(shift=0)),
        (ERR_ARG, dict(d_out=d_in)),                          # in place
        (ERR_ARG, dict(d_out=d_in + 32 * (n - 1))),           # the last input row
        (ERR_ARG, dict(d_in=d_out + 32 * (n - 1), in_len=1, in_rows=1)),  # inside the output
        (ERR_ARG, dict(n_cols=2, in_rows=2 * n)),             # the second column's stride reaches it
        (ERR_ROWS, dict(in_len=n + 1, in_rows=n + 1)),
        (ERR_ROWS, dict(in_rows=n - 1)),
        (ERR_ROWS, dict(out_rows=n - 1)),
    ]
    for code, kw in table:
        with pytest.raises(B2FError) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value)
    # null omega / shift: the wrapper cannot pass them
    lib, vp = engine.lib, ctypes.c_void_p
    for om, sh in ((None, _limbs4(1)), (_limbs4(w), None)):
        rc = lib.b2f_ntt_columns_dev(engine.ctx, vp(d_in), n, n, 1, k, om, sh, FWD, form, vp(d_out), n,
                                     vp(_stream()))
        assert rc == ERR_ARG
    assert lib.b2f_ntt_columns_dev(None, vp(d_in), n, n, 1, k, _limbs4(w), _limbs4(1), FWD, form,
                                   vp(d_out), n, vp(_stream())) == ERR_ARG
    engine.sync(_stream())
    assert torch.equal(buf, before)  # nothing was launched
    # adjacent, not overlapping: accepted
    call(d_out=d_in + 32 * n)
    engine.sync(_stream())
    want = nr.pack(nr.forward(vals, k, w, 1, p), form)
    assert _first_diff(_host(buf[n:2 * n]), want) is None
    assert torch.equal(buf[2 * n:], before[2 * n:])


def test_a_generator_of_the_wrong_order_raises_at_sync(engine):
    from b2f import B2FError

    form, k = 2, 9
    p = nr.modulus(form)
    n = 1 << k
    rng = np.random.default_rng(81)
    vals = nr.random_elements(rng, n, p)
    x = nr.pack(vals, form)[None]
    shift = _shift(rng, p)
    for direction in (FWD, INV):
        for bad in (_omega(form, k - 1), 1, 0, _omega(form, k + 1), _omega(form, k - 1)):
            with pytest.raises(B2FError) as e:
                _run(engine, x, n, k, direction, shift, form, omega=bad)
            assert e.value.code == ERR_FIELD, (direction, bad)
            got = _run(engine, x, n, k, direction, shift, form)  # syncs clean
            assert _first_diff(got[0], nr.pack(_expect(vals, n, k, direction, shift, form), form)) is None


# ---------------------------------------------------------------------------------------------
# 9. timing


def test_one_call_is_one_timed_region(engine):
    form, k = 1, 13
    x = _random_device(3, 1 << k, 90)
    engine.sync(_stream())
    engine.set_timing(True)
    try:
        engine.ntt_columns(x, k, shift=5, form=form)
        engine.sync(_stream())
        times = engine.kernel_times()
    finally:
        engine.set_timing(False)
    assert times["ntt"][1] == 1 and times["ntt"][0] > 0
    assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "ntt")
