"""b2f_lagrange_selectors_dev, b2f_quotient_permutation_dev, b2f_quotient_lookup_dev and
b2f_quotient_divide_dev against the big-integer reference (tests/quotient_ref.py, which
tests/test_quotient_ref.py pins by the arguments' own property). Every comparison is bit-exact.

  1  selectors: k = 1..6, usable_rows from 0 to 2^k - 1, every form, every row, padded stride;
  2  the permutation terms on random columns, every row: (k, ext_k) in {(1,2), (2,5), (3,4), (5,7)}
     in all four forms and (10,12) in the Montgomery form of each field; chunk_len in {1, 2, 3, 5, 8};
     usable_rows in {0, 1, n - 6, n - 1}; rows > n_ext; h_in NULL, given, in place;
  3  the lookup terms the same way;
  4  the divide: every row, in place and not; shift = 1 and a non-primitive omega_ext raise
     B2F_ERR_FIELD at sync and the next call works;
  5  the library's own permutation columns at k = 10, ext_k = 12: the quotient has no coefficient
     of index >= 3n - 3, an altered z cell gives some, sampled rows equal the reference;
  6  the same for the lookup at k = 17, ext_k = 19, and both arguments chained into one h;
  7  every argument error of the header, nothing launched, then a good call;
  8  each call is exactly one `quotient` timed region.

Needs an MI355X (`-m gpu`)."""
import ctypes

import numpy as np
import pytest

import ntt_ref as nr
import quotient_ref as qr

from conftest import random_inputs

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ROWS, ERR_FIELD = 1, 3, 7
SMALL = [(1, 2), (2, 5), (3, 4), (5, 7)]
CHUNKS = [1, 2, 3, 5, 8]
PAD = 5  # pattern rows after the n_ext rows of every column


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _field(form):
    from b2f import field

    return field.of_form(form)


def _omega(form, k):
    from b2f import field

    return field.omega(_field(form), k)


def _delta(form):
    from b2f import field

    return field.delta(_field(form))


def _zeta(form):
    """A cube root of unity: halo2's coset generator F::ZETA is one."""
    from b2f import field

    f, p = _field(form), nr.modulus(form)
    z = pow(field.GENERATOR[f], (p - 1) // 3, p)
    assert z != 1 and pow(z, 3, p) == 1
    return z


def _pattern(shape):
    return np.full(shape, 0xA5A5A5A5DEADBEEF, dtype=np.uint64)


def _usables(k):
    n = 1 << k
    return sorted({u for u in (0, 1, n - 6, n - 1) if 0 <= u < n})


def _block(cols, form, rows):
    """Columns of ints as device limbs [n_cols, rows, 4]; rows past the data hold the pattern."""
    out = _pattern((len(cols), rows, 4))
    for c, col in enumerate(cols):
        out[c, :len(col)] = nr.pack(col, form)
    return _dev(out)


def _first_diff(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return int(bad[0]) if len(bad) else None


class Problem:
    """Random extended columns of one (k, ext_k, form), on the host as ints and on the device."""

    def __init__(self, k, ext_k, form, seed):
        self.k, self.ext_k, self.form = k, ext_k, form
        self.p = nr.modulus(form)
        self.n_ext = 1 << ext_k
        self.rows = self.n_ext + PAD
        rng = np.random.default_rng(seed)
        rand = lambda count: [nr.random_elements(rng, self.n_ext, self.p) for _ in range(count)]  # noqa: E731
        self.l, self.adv, self.sigma, self.z, self.lk = rand(3), rand(10), rand(8), rand(8), rand(5)
        # the special values ride along
        self.l[0][0], self.l[1][1 % self.n_ext], self.z[0][0] = 0, 1, 1
        self.adv[3][self.n_ext - 1] = self.p - 1
        self.h_in = nr.random_elements(rng, self.n_ext, self.p)
        self.beta, self.gamma, self.y = nr.random_elements(rng, 3, self.p)
        self.omega_ext, self.shift, self.delta = _omega(form, ext_k), _zeta(form), _delta(form)
        self.d_l, self.d_adv = _block(self.l, form, self.rows), _block(self.adv, form, self.rows)
        self.d_sigma, self.d_z = _block(self.sigma, form, self.rows), _block(self.z, form, self.rows)
        self.d_lk = _block(self.lk, form, self.rows)

    def v(self):
        import b2f

        return [self.adv[b2f.halo2_column_index(j + 1)] for j in range(8)]

    def h_buffers(self, mode):
        """(d_h_in or None, d_h_out, host h_in or None) for mode 0 NULL, 1 given, 2 in place."""
        h_in = _block([self.h_in], self.form, self.rows)[0]
        if mode == 0:
            return None, _dev(_pattern((self.rows, 4))), None
        if mode == 1:
            return h_in, _dev(_pattern((self.rows, 4))), self.h_in
        return h_in, h_in, self.h_in

    def check_h(self, d_out, want, label):
        got = _host(d_out)
        bad = _first_diff(got[:self.n_ext], nr.pack(want, self.form))
        assert bad is None, (label, "row %d" % bad)
        assert (got[self.n_ext:] == _pattern((PAD, 4))).all(), label

    def run_permutation(self, engine, chunk_len, usable, mode):
        sets = -(-8 // chunk_len)
        h_in, h_out, host_in = self.h_buffers(mode)
        engine.quotient_permutation_dev(self.k, self.ext_k, usable, self.d_l.data_ptr(), self.d_adv.data_ptr(),
                                        self.d_sigma.data_ptr(), self.d_z.data_ptr(), chunk_len, self.rows,
                                        self.omega_ext, self.shift, self.delta, self.beta, self.gamma, self.y,
                                        h_in.data_ptr() if h_in is not None else 0, h_out.data_ptr(),
                                        self.form, _stream())
        engine.sync(_stream())
        terms = qr.permutation_terms(self.k, self.ext_k, usable, self.l, self.v(), self.sigma, self.z[:sets],
                                     chunk_len, self.omega_ext, self.shift, self.delta, self.beta, self.gamma,
                                     self.p)
        assert len(terms) == 2 * sets + 1
        self.check_h(h_out, qr.fold(terms, self.y, self.p, host_in), (chunk_len, usable, mode))

    def run_lookup(self, engine, mode):
        h_in, h_out, host_in = self.h_buffers(mode)
        engine.quotient_lookup_dev(self.k, self.ext_k, self.d_l.data_ptr(), self.d_lk.data_ptr(), self.rows,
                                   self.beta, self.gamma, self.y, h_in.data_ptr() if h_in is not None else 0,
                                   h_out.data_ptr(), self.form, _stream())
        engine.sync(_stream())
        terms = qr.lookup_terms(self.k, self.ext_k, self.l, self.lk, self.beta, self.gamma, self.p)
        self.check_h(h_out, qr.fold(terms, self.y, self.p, host_in), ("lookup", mode))

    def run_divide(self, engine, in_place):
        h_in, h_out, _ = self.h_buffers(2 if in_place else 1)
        engine.quotient_divide_dev(self.k, self.ext_k, self.omega_ext, self.shift, h_in.data_ptr(),
                                   h_out.data_ptr(), self.form, _stream())
        engine.sync(_stream())
        self.check_h(h_out, qr.divide(self.h_in, self.k, self.ext_k, self.omega_ext, self.shift, self.p),
                     ("divide", in_place))


# ---------------------------------------------------------------------------------------------
# 1. selectors


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_selectors_every_row(engine, form):
    for k in range(1, 7):
        n = 1 << k
        for usable in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
            out_rows = n + 3
            d_out = _dev(_pattern((3, out_rows, 4)))
            engine.lagrange_selectors_dev(k, usable, form, d_out.data_ptr(), out_rows, _stream())
            engine.sync(_stream())
            got = _host(d_out)
            for c, col in enumerate(qr.selectors(k, usable)):
                assert _first_diff(got[c, :n], nr.pack(col, form)) is None, (k, usable, c)
                assert (got[c, n:] == _pattern((3, 4))).all(), (k, usable, c)
    t = engine.lagrange_selectors(3, 5, form=form)
    engine.sync(_stream())
    assert tuple(t.shape) == (3, 8, 4)
    assert [nr.unpack(c, form) for c in _host(t)] == [list(c) for c in qr.selectors(3, 5)]


# ---------------------------------------------------------------------------------------------
# 2. permutation terms on random columns


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", SMALL)
def test_permutation_terms_small(engine, shape, form):
    k, ext_k = shape
    pr = Problem(k, ext_k, form, 100 + 10 * k + form)
    mode = 0
    for chunk_len in CHUNKS:
        for usable in _usables(k):
            pr.run_permutation(engine, chunk_len, usable, mode % 3)
            mode += 1
        mode += 1  # every chunk_len meets another order of the three h modes


@pytest.mark.parametrize("chunk_len", CHUNKS)
@pytest.mark.parametrize("form", [1, 3])
def test_permutation_terms_across_blocks_and_tables(engine, form, chunk_len):
    pr = Problem(10, 12, form, 200 + form)
    for mode, usable in enumerate(_usables(10)):
        pr.run_permutation(engine, chunk_len, usable, (mode + chunk_len) % 3)


# ---------------------------------------------------------------------------------------------
# 3. lookup terms on random columns


@pytest.mark.parametrize("shape,form", [(sh, f) for sh in SMALL for f in (0, 1, 2, 3)] + [((10, 12), 1), ((10, 12), 3)])
def test_lookup_terms(engine, shape, form):
    k, ext_k = shape
    pr = Problem(k, ext_k, form, 300 + 10 * k + form)
    for mode in range(3):
        pr.run_lookup(engine, mode)


# ---------------------------------------------------------------------------------------------
# 4. divide


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_divide_every_row(engine, form):
    for k, ext_k in SMALL + ([(10, 12)] if form & 1 else []):
        pr = Problem(k, ext_k, form, 400 + 10 * k + form)
        pr.run_divide(engine, False)
        pr.run_divide(engine, True)


@pytest.mark.parametrize("form", [1, 2])
def test_vanishing_point_and_wrong_root_raise_at_sync(engine, form):
    from b2f import B2FError

    k, ext_k = 3, 5
    pr = Problem(k, ext_k, form, 450 + form)

    def divide(omega_ext, shift):
        h_in, h_out, _ = pr.h_buffers(1)
        engine.quotient_divide_dev(k, ext_k, omega_ext, shift, h_in.data_ptr(), h_out.data_ptr(), form, _stream())
        engine.sync(_stream())

    for omega_ext, shift in ((pr.omega_ext, 1),                      # X_0^n = 1
                             (pr.omega_ext, _omega(form, k)),        # shift in the domain: the same
                             (_omega(form, ext_k - 1), pr.shift),    # not primitive
                             (1, pr.shift), (0, pr.shift)):
        for _ in range(2):  # the second call finds the domain's divisors cached, and raises again
            with pytest.raises(B2FError) as e:
                divide(omega_ext, shift)
            assert e.value.code == ERR_FIELD, (omega_ext, shift)
        pr.run_divide(engine, True)  # syncs clean, right result
    # the permutation call checks the root too (and caches the table of the bad root apart)
    for bad in (_omega(form, ext_k - 1), 1):
        _, h_out, _ = pr.h_buffers(0)
        with pytest.raises(B2FError) as e:
            engine.quotient_permutation_dev(k, ext_k, 2, pr.d_l.data_ptr(), pr.d_adv.data_ptr(),
                                            pr.d_sigma.data_ptr(), pr.d_z.data_ptr(), 3, pr.rows, bad, pr.shift,
                                            pr.delta, pr.beta, pr.gamma, pr.y, 0, h_out.data_ptr(), form,
                                            _stream())
            engine.sync(_stream())
        assert e.value.code == ERR_FIELD
        pr.run_permutation(engine, 3, 2, 1)


# ---------------------------------------------------------------------------------------------
# 5, 6. the library's own columns


def _random_rows(shape, seed):
    """Dense random elements < 2^253 (below both moduli: a valid element in any form)."""
    import torch

    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    x = torch.randint(0, 2**32, shape, dtype=torch.int64, device="cuda:0", generator=g) << 32
    x |= torch.randint(0, 2**32, shape, dtype=torch.int64, device="cuda:0", generator=g)
    x[..., 3] &= (1 << 61) - 1
    return x


def _gather(t, idx, form):
    """Columns of the device tensor t [n_cols, rows, 4] as dicts {extended row: value}."""
    import torch

    sel = _host(t[:, torch.tensor(idx, device="cuda:0")])
    return [dict(zip(idx, nr.unpack(col, form))) for col in sel]


def _neighbours(rows, n_ext, rot, usable):
    return sorted({(i + d) % n_ext for i in rows for d in (0, rot, -rot, usable * rot)})


def _high_coefficients_zero(engine, h, k, ext_k, shift, form):
    """Divide a copy of the numerator h by X^n - 1, interpolate on the coset, and say on the
    device whether every coefficient of index >= 3n - 3 is zero."""
    q = engine.quotient_divide(k, ext_k, shift, h.clone(), form=form)
    coeff = engine.ntt_columns(q[None], ext_k, inverse=True, shift=shift, form=form)
    engine.sync(_stream())
    return q, bool((coeff[0, 3 * (1 << k) - 3:] == 0).all())


class Circuit:
    """One circuit of the library's own columns in a 2^k-row domain, extended to 2^ext_k."""

    def __init__(self, engine, x, k, ext_k, form, chunk_len, seed):
        import b2f

        self.engine, self.k, self.ext_k, self.form, self.chunk_len = engine, k, ext_k, form, chunk_len
        self.p = nr.modulus(form)
        self.n, self.n_ext = 1 << k, 1 << ext_k
        self.usable = self.n - 6
        self.shift = _zeta(form)
        rng = np.random.default_rng(seed)
        self.beta, self.gamma, self.y, self.theta = nr.random_elements(rng, 4, self.p)
        self.batch = b2f.DeviceBatch(x)
        self.batch.fill(engine)
        self.used = int(self.batch.offsets_host[-1])
        assert self.used <= self.usable
        self.l = self.extend(engine.lagrange_selectors(k, self.usable, form=form))
        self.seed = seed

    def extend(self, cols):
        return self.engine.extend_columns(cols, self.k, self.ext_k, self.shift, form=self.form)

    def permutation_columns(self):
        import torch

        adv = torch.zeros((10, self.n, 4), dtype=torch.int64, device="cuda:0")
        self.batch.export_fp(self.engine, 0, self.used, form=self.form, out=adv)
        adv[:, self.usable:] = _random_rows((10, self.n - self.usable, 4), self.seed + 1)  # blinding rows
        sigma, z = self.batch.permutation_columns(self.engine, self.k, self.usable, self.beta, self.gamma,
                                                  chunk_len=self.chunk_len, form=self.form)
        z[:, self.usable + 1:] = _random_rows((z.shape[0], self.n - self.usable - 1, 4), self.seed + 2)
        self.z_lagrange = z
        self.adv, self.sigma, self.z = self.extend(adv), self.extend(sigma), self.extend(z)

    def lookup_columns(self):
        import torch

        cols = torch.zeros((5, self.n, 4), dtype=torch.int64, device="cuda:0")
        begin = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        bad = torch.empty(1, dtype=torch.int64, device="cuda:0")
        self.engine.lookup_columns_dev(self.batch.advice.data_ptr(), self.batch.total_rows, begin.data_ptr(), 1,
                                       self.usable, self.theta, self.beta, self.gamma, self.form, cols.data_ptr(),
                                       self.n, bad.data_ptr(), _stream())
        cols[:4, self.usable:] = _random_rows((4, self.n - self.usable, 4), self.seed + 3)  # blinding rows
        cols[4, self.usable + 1:] = _random_rows((self.n - self.usable - 1, 4), self.seed + 4)
        self.engine.sync(_stream())
        assert int(bad[0]) == -1  # UINT64_MAX: every input row is a table row
        self.lookup_lagrange = cols
        self.lookup = self.extend(cols)

    def permutation_h(self, h=None):
        return self.engine.quotient_permutation(self.k, self.ext_k, self.usable, self.l, self.adv, self.sigma,
                                                self.z, self.chunk_len, self.shift, self.beta, self.gamma, self.y,
                                                h=h, form=self.form)

    def lookup_h(self, h=None):
        return self.engine.quotient_lookup(self.k, self.ext_k, self.l, self.lookup, self.beta, self.gamma, self.y,
                                           h=h, form=self.form)

    def sample(self, count):
        rng = np.random.default_rng(self.seed + 5)
        rows = sorted({0, 1, self.n_ext - 1} | {int(r) for r in rng.integers(0, self.n_ext, count - 3)})
        return rows, _neighbours(rows, self.n_ext, self.n_ext // self.n, self.usable)

    def permutation_reference(self, rows, near):
        import b2f

        adv = _gather(self.adv, near, self.form)
        return qr.permutation_terms(self.k, self.ext_k, self.usable, _gather(self.l, near, self.form),
                                    [adv[b2f.halo2_column_index(j + 1)] for j in range(8)],
                                    _gather(self.sigma, near, self.form), _gather(self.z, near, self.form),
                                    self.chunk_len, _omega(self.form, self.ext_k), self.shift, _delta(self.form),
                                    self.beta, self.gamma, self.p, rows=rows)

    def lookup_reference(self, rows, near):
        return qr.lookup_terms(self.k, self.ext_k, _gather(self.l, near, self.form),
                               _gather(self.lookup, near, self.form), self.beta, self.gamma, self.p, rows=rows)

    def rows_of(self, h, rows):
        import torch

        return nr.unpack(_host(h[torch.tensor(rows, device="cuda:0")]), self.form)


def test_own_permutation_columns_divide_exactly(engine):
    form, k, ext_k = 1, 10, 12
    x = random_inputs(2, (0,), 61)
    x["rounds"] = np.asarray([1, 0], dtype=np.uint32)
    c = Circuit(engine, x, k, ext_k, form, 2, 500)
    assert c.used == 872
    c.permutation_columns()
    h = c.permutation_h()
    q, zero = _high_coefficients_zero(engine, h, k, ext_k, c.shift, form)
    assert zero
    rows, near = c.sample(64)
    want = qr.fold(c.permutation_reference(rows, near), c.y, c.p)
    assert c.rows_of(h, rows) == want
    assert c.rows_of(q, rows) == qr.divide(want, k, ext_k, _omega(form, ext_k), c.shift, c.p, rows)
    # one altered z cell: the numerator is no multiple of X^n - 1 any more
    z = c.z_lagrange.clone()
    z[1, 5, 0] ^= 1
    c.z = c.extend(z)
    _, zero = _high_coefficients_zero(engine, c.permutation_h(), k, ext_k, c.shift, form)
    assert not zero


def test_own_lookup_columns_divide_exactly_and_chain_with_the_permutation(engine):
    form, k, ext_k = 3, 17, 19
    c = Circuit(engine, random_inputs(5, (12,), 62), k, ext_k, form, 2, 600)
    c.lookup_columns()
    h = c.lookup_h()
    q, zero = _high_coefficients_zero(engine, h, k, ext_k, c.shift, form)
    assert zero
    rows, near = c.sample(64)
    lk_terms = c.lookup_reference(rows, near)
    want = qr.fold(lk_terms, c.y, c.p)
    assert c.rows_of(h, rows) == want
    assert c.rows_of(q, rows) == qr.divide(want, k, ext_k, _omega(form, ext_k), c.shift, c.p, rows)
    del h, q
    # permutation then lookup into one h with one y, halo2's order
    c.permutation_columns()
    h = c.permutation_h()
    assert c.lookup_h(h=h) is h
    _, zero = _high_coefficients_zero(engine, h, k, ext_k, c.shift, form)
    assert zero
    assert c.rows_of(h, rows) == qr.fold(c.permutation_reference(rows, near) + lk_terms, c.y, c.p)
    del h
    # one altered z cell of the lookup
    cols = c.lookup_lagrange.clone()
    cols[4, 77, 0] ^= 1
    c.lookup = c.extend(cols)
    _, zero = _high_coefficients_zero(engine, c.lookup_h(), k, ext_k, c.shift, form)
    assert not zero


# ---------------------------------------------------------------------------------------------
# 7. errors


def _limbs4(v):
    return (ctypes.c_uint64 * 4)(*[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)])


def _expect_errors(table, call):
    from b2f import B2FError

    for code, kw in table:
        with pytest.raises(B2FError) as e:
            call(**kw)
        assert e.value.code == code, (kw, e.value)


def test_argument_errors_then_good_calls(engine):
    import torch

    form, k, ext_k = 1, 3, 5
    pr = Problem(k, ext_k, form, 700)
    p, n_ext, rows = pr.p, pr.n_ext, pr.rows
    # every block in one buffer, so "unchanged" covers all of them
    sizes = [("l", 3 * rows), ("adv", 10 * rows), ("sigma", 8 * rows), ("z", 8 * rows), ("lk", 5 * rows),
             ("h_in", n_ext), ("h_out", n_ext), ("sel", 3 * 8)]
    buf = torch.empty((sum(s for _, s in sizes), 4), dtype=torch.int64, device="cuda:0")
    at, off = {}, 0
    for name, size in sizes:
        at[name] = buf.data_ptr() + 32 * off
        src = {"l": pr.d_l, "adv": pr.d_adv, "sigma": pr.d_sigma, "z": pr.d_z, "lk": pr.d_lk}.get(name)
        if src is not None:
            buf[off:off + size] = src.reshape(-1, 4)
        elif name == "h_in":
            buf[off:off + size] = _dev(nr.pack(pr.h_in, form))
        else:
            buf[off:off + size] = 0x5A5A5A5A
        off += size
    before = buf.clone()
    s = _stream()

    good_p = dict(k=k, ext_k=ext_k, usable=2, d_l=at["l"], d_advice=at["adv"], d_sigma=at["sigma"], d_z=at["z"],
                  chunk_len=3, rows=rows, omega_ext=pr.omega_ext, shift=pr.shift, delta=pr.delta, beta=pr.beta,
                  gamma=pr.gamma, y=pr.y, d_h_in=at["h_in"], d_h_out=at["h_out"], form=form)

    def perm(**kw):
        a = dict(good_p, **kw)
        engine.quotient_permutation_dev(a["k"], a["ext_k"], a["usable"], a["d_l"], a["d_advice"], a["d_sigma"],
                                        a["d_z"], a["chunk_len"], a["rows"], a["omega_ext"], a["shift"],
                                        a["delta"], a["beta"], a["gamma"], a["y"], a["d_h_in"], a["d_h_out"],
                                        a["form"], s)

    common = [(ERR_ARG, dict(d_l=0)), (ERR_ARG, dict(d_h_out=0)),
              (ERR_ARG, dict(d_l=at["l"] + 8)), (ERR_ARG, dict(d_h_in=at["h_in"] + 8)),
              (ERR_ARG, dict(d_h_out=at["h_out"] + 8)),
              (ERR_ARG, dict(k=0)), (ERR_ARG, dict(k=ext_k)), (ERR_ARG, dict(k=ext_k + 1)),
              (ERR_ARG, dict(ext_k=29, rows=1 << 29)), (ERR_ARG, dict(form=4)),
              (ERR_ARG, dict(beta=p)), (ERR_ARG, dict(gamma=p)), (ERR_ARG, dict(y=2**256 - 1)),
              (ERR_ARG, dict(d_h_in=at["h_out"] + 32)),              # h_in inside h_out, not equal
              (ERR_ARG, dict(d_h_in=at["h_out"] - 32 * (n_ext - 1))),
              (ERR_ARG, dict(d_h_out=at["l"])),                      # h_out on the first selector row
              (ERR_ARG, dict(d_h_out=at["l"] + 32 * (3 * rows - 1))),  # ... and on the block's last row
              (ERR_ROWS, dict(rows=n_ext - 1))]
    _expect_errors(common + [
        (ERR_ARG, dict(d_advice=0)), (ERR_ARG, dict(d_sigma=0)), (ERR_ARG, dict(d_z=0)),
        (ERR_ARG, dict(d_advice=at["adv"] + 8)), (ERR_ARG, dict(d_sigma=at["sigma"] + 8)),
        (ERR_ARG, dict(d_z=at["z"] + 8)),
        (ERR_ARG, dict(chunk_len=0)), (ERR_ARG, dict(chunk_len=9)),
        (ERR_ARG, dict(omega_ext=p)), (ERR_ARG, dict(shift=p)), (ERR_ARG, dict(delta=p)),
        (ERR_ARG, dict(shift=0)),
        (ERR_ARG, dict(d_h_out=at["adv"] + 32 * rows)), (ERR_ARG, dict(d_h_out=at["sigma"] + 32 * 7 * rows)),
        (ERR_ARG, dict(d_h_out=at["z"] + 32 * 2 * rows)),       # the last of chunk_len 3's three z columns
        (ERR_ROWS, dict(usable=1 << k)), (ERR_ROWS, dict(usable=2**40)),
    ], perm)

    good_l = dict(k=k, ext_k=ext_k, d_l=at["l"], d_lookup=at["lk"], rows=rows, beta=pr.beta, gamma=pr.gamma,
                  y=pr.y, d_h_in=at["h_in"], d_h_out=at["h_out"], form=form)

    def lookup(**kw):
        a = dict(good_l, **kw)
        engine.quotient_lookup_dev(a["k"], a["ext_k"], a["d_l"], a["d_lookup"], a["rows"], a["beta"], a["gamma"],
                                   a["y"], a["d_h_in"], a["d_h_out"], a["form"], s)

    _expect_errors(common + [(ERR_ARG, dict(d_lookup=0)), (ERR_ARG, dict(d_lookup=at["lk"] + 8)),
                             (ERR_ARG, dict(d_h_out=at["lk"] + 32 * 4 * rows))], lookup)

    good_d = dict(k=k, ext_k=ext_k, omega_ext=pr.omega_ext, shift=pr.shift, d_h_in=at["h_in"],
                  d_h_out=at["h_out"], form=form)

    def divide(**kw):
        a = dict(good_d, **kw)
        engine.quotient_divide_dev(a["k"], a["ext_k"], a["omega_ext"], a["shift"], a["d_h_in"], a["d_h_out"],
                                   a["form"], s)

    _expect_errors([(ERR_ARG, dict(d_h_in=0)), (ERR_ARG, dict(d_h_out=0)),
                    (ERR_ARG, dict(d_h_in=at["h_in"] + 8)), (ERR_ARG, dict(d_h_out=at["h_out"] + 8)),
                    (ERR_ARG, dict(k=0)), (ERR_ARG, dict(k=ext_k)), (ERR_ARG, dict(ext_k=29)),
                    (ERR_ARG, dict(form=4)), (ERR_ARG, dict(omega_ext=p)), (ERR_ARG, dict(shift=p)),
                    (ERR_ARG, dict(shift=0)), (ERR_ARG, dict(d_h_in=at["h_out"] + 32))], divide)

    good_s = dict(k=3, usable=5, form=form, d_out=at["sel"], out_rows=8)

    def selectors(**kw):
        a = dict(good_s, **kw)
        engine.lagrange_selectors_dev(a["k"], a["usable"], a["form"], a["d_out"], a["out_rows"], s)

    _expect_errors([(ERR_ARG, dict(d_out=0)), (ERR_ARG, dict(d_out=at["sel"] + 8)), (ERR_ARG, dict(k=0)),
                    (ERR_ARG, dict(k=29, out_rows=1 << 29)), (ERR_ARG, dict(form=4)),
                    (ERR_ROWS, dict(usable=8)), (ERR_ROWS, dict(out_rows=7))], selectors)

    # null challenge pointers and null contexts: the wrappers cannot pass them
    lib, vp = engine.lib, ctypes.c_void_p
    el = [_limbs4(v) for v in (pr.omega_ext, pr.shift, pr.delta, pr.beta, pr.gamma, pr.y)]
    ptrs = [vp(at[n]) for n in ("l", "adv", "sigma", "z")]
    for ctx, hole, want in [(engine.ctx, i, ERR_ARG) for i in range(6)] + [(None, None, ERR_ARG)]:
        e = [None if i == hole else v for i, v in enumerate(el)]
        assert lib.b2f_quotient_permutation_dev(ctx, k, ext_k, 2, *ptrs, 3, rows, *e, vp(at["h_in"]),
                                                vp(at["h_out"]), form, vp(s)) == want
    for ctx, hole in [(engine.ctx, i) for i in range(3)] + [(None, None)]:
        e = [None if i == hole else v for i, v in enumerate(el[3:])]
        assert lib.b2f_quotient_lookup_dev(ctx, k, ext_k, vp(at["l"]), vp(at["lk"]), rows, *e, vp(at["h_in"]),
                                           vp(at["h_out"]), form, vp(s)) == ERR_ARG
    for ctx, om, sh in ((engine.ctx, None, el[1]), (engine.ctx, el[0], None), (None, el[0], el[1])):
        assert lib.b2f_quotient_divide_dev(ctx, k, ext_k, om, sh, vp(at["h_in"]), vp(at["h_out"]), form,
                                           vp(s)) == ERR_ARG
    assert lib.b2f_lagrange_selectors_dev(None, 3, 5, form, vp(at["sel"]), 8, vp(s)) == ERR_ARG
    engine.sync(s)
    assert torch.equal(buf, before)  # nothing was launched

    # good calls: each writes its own block and nothing else
    def block(name):
        o = (at[name] - buf.data_ptr()) // 32
        return buf[o:o + dict(sizes)[name]]

    perm()
    engine.sync(s)
    terms = qr.permutation_terms(k, ext_k, 2, pr.l, pr.v(), pr.sigma, pr.z[:3], 3, pr.omega_ext, pr.shift,
                                 pr.delta, pr.beta, pr.gamma, p)
    h = qr.fold(terms, pr.y, p, pr.h_in)
    assert _first_diff(_host(block("h_out")), nr.pack(h, form)) is None
    lookup(d_h_in=at["h_out"])  # in place, on top
    engine.sync(s)
    h = qr.fold(qr.lookup_terms(k, ext_k, pr.l, pr.lk, pr.beta, pr.gamma, p), pr.y, p, h)
    assert _first_diff(_host(block("h_out")), nr.pack(h, form)) is None
    divide(d_h_in=at["h_out"])
    selectors()
    engine.sync(s)
    h = qr.divide(h, k, ext_k, pr.omega_ext, pr.shift, p)
    assert _first_diff(_host(block("h_out")), nr.pack(h, form)) is None
    assert [nr.unpack(c, form) for c in _host(block("sel")).reshape(3, 8, 4)] == \
        [list(c) for c in qr.selectors(3, 5)]
    o = (at["h_out"] - buf.data_ptr()) // 32
    assert torch.equal(buf[:o], before[:o])  # every input block is as it was


# ---------------------------------------------------------------------------------------------
# 8. timing


def test_each_call_is_one_timed_region(engine):
    form, k, ext_k = 3, 5, 7
    pr = Problem(k, ext_k, form, 800)
    s = _stream()

    def perm():
        pr.run_permutation(engine, 2, 7, 1)

    def lookup():
        pr.run_lookup(engine, 2)

    def divide():
        pr.run_divide(engine, True)

    for call in (perm, lookup, divide):
        engine.sync(s)
        engine.set_timing(True)
        try:
            call()
            times = engine.kernel_times()
        finally:
            engine.set_timing(False)
        assert times["quotient"][1] == 1 and times["quotient"][0] > 0, call.__name__
        assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "quotient"), call.__name__
