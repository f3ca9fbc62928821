"""tests/quotient_ref.py pinned by the arguments' own property, on the CPU.

A toy permutation argument and a toy lookup argument at k = 4, ext_k = 6 are built by their
definitions with random blinding rows, taken to the coset with tests/ntt_ref.py, folded, divided
by X^n - 1 and interpolated back. Every term of a valid argument vanishes on the 2^k domain, so the
numerator (degree <= (chunk_len + 2)(n - 1) for the permutation with chunk_len = 2, 4(n - 1) for
the lookup) is a multiple of X^n - 1 and the quotient has degree <= 3n - 4: every coefficient of
index >= 3n - 3 is zero. An argument with one broken z cell, one broken copy or one broken
permuted cell is no multiple, and some of those coefficients are not zero."""
import numpy as np
import pytest

import ntt_ref as nr
import quotient_ref as qr

K, EXT_K = 4, 6
N, N_EXT = 1 << K, 1 << EXT_K
USABLE = 10  # 5 blinding rows
CHUNK = 2
FORM = 1
P = nr.modulus(FORM)


def _field():
    from b2f import field

    f = field.of_form(FORM)
    return field.omega(f, K), field.omega(f, EXT_K), field.delta(f), pow(field.GENERATOR[f], (P - 1) // 3, P)


def _inv(x):
    return pow(x, P - 2, P)


def toy_permutation(rng, beta, gamma, omega, delta):
    """(v, sigma, z): eight columns with a few copy cycles, sigma and the chained grand products
    by the definition of include/b2f.h (b2f_permutation_columns_dev), random blinding rows."""
    v = [nr.random_elements(rng, N, P) for _ in range(8)]
    cycles = [[(0, 1), (3, 7), (7, 2)], [(2, 0), (2, 9)], [(5, 4), (1, 4), (6, 8), (0, 5)]]
    mapping = {(j, i): (j, i) for j in range(8) for i in range(N)}
    for cyc in cycles:
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            mapping[a] = b
            v[b[0]][b[1]] = v[cyc[0][0]][cyc[0][1]]
    sigma = [[pow(delta, mapping[(j, i)][0], P) * pow(omega, mapping[(j, i)][1], P) % P for i in range(N)]
             for j in range(8)]
    z, start = [], 1
    for s in range(8 // CHUNK):
        col = [start]
        for i in range(USABLE):
            num = den = 1
            for j in range(s * CHUNK, (s + 1) * CHUNK):
                num = num * (v[j][i] + beta * pow(delta, j, P) * pow(omega, i, P) + gamma) % P
                den = den * (v[j][i] + beta * sigma[j][i] + gamma) % P
            col.append(col[-1] * num * _inv(den) % P)
        start = col[USABLE]
        z.append(col + nr.random_elements(rng, N - USABLE - 1, P))
    assert z[-1][USABLE] == 1
    return v, sigma, z


def toy_lookup(rng, beta, gamma):
    """(A, S, A', S', z): 10 inputs into a 6-row table (padded with its row 0 to the usable rows),
    permuted by halo2's rule, z by the definition, random blinding rows."""
    table = nr.random_elements(rng, 6, P)
    s_col = table + [table[0]] * (USABLE - 6)
    a_col = [table[int(t)] for t in rng.integers(0, 6, USABLE)]
    ap = sorted(a_col)
    sp, spare = [None] * USABLE, list(s_col)
    for i in range(USABLE):
        if i == 0 or ap[i] != ap[i - 1]:
            sp[i] = ap[i]
            spare.remove(ap[i])
    for i in range(USABLE):
        if sp[i] is None:
            sp[i] = spare.pop()
    assert sorted(sp) == sorted(s_col)
    z = [1]
    for i in range(USABLE):
        num = (a_col[i] + beta) * (s_col[i] + gamma) % P
        den = (ap[i] + beta) * (sp[i] + gamma) % P
        z.append(z[-1] * num * _inv(den) % P)
    assert z[USABLE] == 1
    blind = lambda c, used: c + nr.random_elements(rng, N - used, P)  # noqa: E731
    return [blind(a_col, USABLE), blind(s_col, USABLE), blind(ap, USABLE), blind(sp, USABLE),
            blind(z, USABLE + 1)]


class Toy:
    def __init__(self):
        rng = np.random.default_rng(7)
        self.omega, self.omega_ext, self.delta, self.shift = _field()
        self.beta, self.gamma, self.y = nr.random_elements(rng, 3, P)
        self.v, self.sigma, self.z = toy_permutation(rng, self.beta, self.gamma, self.omega, self.delta)
        self.lookup = toy_lookup(rng, self.beta, self.gamma)
        self.l = self.ext(qr.selectors(K, USABLE))

    def ext(self, cols):
        return [qr.extend(c, K, EXT_K, self.omega, self.omega_ext, self.shift, P) for c in cols]

    def perm_terms(self, v=None, sigma=None, z=None):
        return qr.permutation_terms(K, EXT_K, USABLE, self.l, self.ext(v or self.v),
                                    self.ext(sigma or self.sigma), self.ext(z or self.z), CHUNK,
                                    self.omega_ext, self.shift, self.delta, self.beta, self.gamma, P)

    def lookup_terms(self, cols=None):
        return qr.lookup_terms(K, EXT_K, self.l, self.ext(cols or self.lookup), self.beta, self.gamma, P)

    def high_coefficients(self, terms):
        h = qr.divide(qr.fold(terms, self.y, P), K, EXT_K, self.omega_ext, self.shift, P)
        return nr.inverse(h, EXT_K, self.omega_ext, self.shift, P)[3 * N - 3:]


@pytest.fixture(scope="module")
def toy():
    return Toy()


def _altered(cols, c, i):
    out = [list(col) for col in cols]
    out[c][i] = (out[c][i] + 1) % P
    return out


def test_selectors():
    l0, llast, lact = qr.selectors(K, USABLE)
    assert sum(l0) == 1 and l0[0] == 1 and sum(llast) == 1 and llast[USABLE] == 1
    assert lact == [1] * USABLE + [0] * (N - USABLE)
    assert qr.selectors(1, 0) == ([1, 0], [1, 0], [0, 0])


def test_valid_permutation_quotient_has_the_low_degree(toy):
    terms = toy.perm_terms()
    assert len(terms) == 2 * 4 + 1 and all(len(t) == N_EXT for t in terms)
    assert any(toy.perm_terms()[-1])  # the terms themselves are not zero off the domain
    assert not any(toy.high_coefficients(terms))


def test_broken_permutation_arguments_are_no_multiple_of_the_vanishing_polynomial(toy):
    assert any(toy.high_coefficients(toy.perm_terms(z=_altered(toy.z, 1, 3))))      # a z cell
    assert any(toy.high_coefficients(toy.perm_terms(z=_altered(toy.z, 3, USABLE))))  # the closing 1
    assert any(toy.high_coefficients(toy.perm_terms(v=_altered(toy.v, 7, 2))))      # a copy
    assert any(toy.high_coefficients(toy.perm_terms(sigma=_altered(toy.sigma, 4, 0))))
    # a blinding row is free
    assert not any(toy.high_coefficients(toy.perm_terms(v=_altered(toy.v, 7, USABLE + 1))))


def test_valid_lookup_quotient_has_the_low_degree(toy):
    terms = toy.lookup_terms()
    assert len(terms) == 5 and any(terms[2])
    assert not any(toy.high_coefficients(terms))
    # both arguments in one accumulator, halo2's order
    assert not any(toy.high_coefficients(toy.perm_terms() + terms))


def test_broken_lookup_arguments_are_no_multiple_of_the_vanishing_polynomial(toy):
    assert any(toy.high_coefficients(toy.lookup_terms(_altered(toy.lookup, 4, 5))))  # a z cell
    assert any(toy.high_coefficients(toy.lookup_terms(_altered(toy.lookup, 2, 4))))  # a permuted input
    assert any(toy.high_coefficients(toy.lookup_terms(_altered(toy.lookup, 3, 0))))  # a permuted table cell
    assert not any(toy.high_coefficients(toy.lookup_terms(_altered(toy.lookup, 0, USABLE))))  # blinding


def test_fold_is_linear_in_the_accumulator(toy):
    terms = toy.perm_terms()
    rng = np.random.default_rng(8)
    h_in = nr.random_elements(rng, N_EXT, P)
    t = len(terms)
    plain = qr.fold(terms, toy.y, P)
    assert qr.fold(terms, toy.y, P, h_in) == [(pow(toy.y, t, P) * a + b) % P for a, b in zip(h_in, plain)]
    # the definition as a sum
    assert plain == [sum(pow(toy.y, t - 1 - i, P) * terms[i][r] for i in range(t)) % P for r in range(N_EXT)]
    # folding two arguments in turn == folding their terms together
    lk = toy.lookup_terms()
    assert qr.fold(lk, toy.y, P, plain) == qr.fold(terms + lk, toy.y, P)


def test_divide_inverts_the_vanishing_polynomial(toy):
    rng = np.random.default_rng(9)
    h = nr.random_elements(rng, N_EXT, P)
    q = qr.divide(h, K, EXT_K, toy.omega_ext, toy.shift, P)
    xs = qr.points(EXT_K, toy.omega_ext, toy.shift, P)
    assert [a * (pow(x, N, P) - 1) % P for a, x in zip(q, xs)] == h
    rows = [5, 63, 0]
    assert qr.divide([h[i] for i in rows], K, EXT_K, toy.omega_ext, toy.shift, P, rows) == [q[i] for i in rows]
    with pytest.raises(AssertionError):
        qr.divide(h, K, EXT_K, toy.omega_ext, 1, P)


def test_sampled_rows_equal_the_full_evaluation(toy):
    rows = [0, 1, 17, 62, 63]
    full = toy.perm_terms()
    ev, es, ez = toy.ext(toy.v), toy.ext(toy.sigma), toy.ext(toy.z)
    part = qr.permutation_terms(K, EXT_K, USABLE, toy.l, ev, es, ez, CHUNK, toy.omega_ext, toy.shift,
                                toy.delta, toy.beta, toy.gamma, P, rows=rows)
    assert part == [[t[i] for i in rows] for t in full]
    lk = toy.ext(toy.lookup)
    assert qr.lookup_terms(K, EXT_K, toy.l, lk, toy.beta, toy.gamma, P, rows=rows) == \
        [[t[i] for i in rows] for t in toy.lookup_terms()]


def test_the_binding_declares_the_four_calls():
    from b2f import _lib

    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"b2f_lagrange_selectors_dev", "b2f_quotient_permutation_dev", "b2f_quotient_lookup_dev",
            "b2f_quotient_divide_dev"} <= names
    assert _lib.KERNEL_NAMES[9] == "quotient" and len(_lib.KERNEL_NAMES) == 10
    import b2f

    for name in ("lagrange_selectors", "extend_columns", "quotient_permutation", "quotient_lookup",
                 "quotient_divide"):
        assert callable(getattr(b2f.Engine, name)), name
