"""Big-integer restatement (Python ints) of the quotient calls of include/b2f.h:
b2f_lagrange_selectors_dev, b2f_quotient_permutation_dev, b2f_quotient_lookup_dev and
b2f_quotient_divide_dev. It depends on tests/ntt_ref.py only.

Everything is defined over extended-coset values. n = 2^k, n_ext = 2^ext_k, rot = 2^(ext_k - k);
extended row i is the point X_i = shift * omega_ext^i, and a rotation by r circuit rows reads
extended row (i + r * rot) mod n_ext. A column is anything indexable by the extended row (a list
of n_ext values, or a dict holding the rows a sampled check touches). usable_rows =
2^k - blinding_factors - 1.

Permutation terms, per row, in this order (halo2_proofs 0.3.0 plonk/permutation/prover.rs,
Committed::construct), with sets = ceil(8 / chunk_len) and T = 2 * sets + 1:

  e_0 = l_0 * (1 - z_0)
  e_1 = l_last * (z_last^2 - z_last), z_last = set sets - 1
  for s = 1 .. sets-1:  l_0 * (z_s - z_{s-1}(w^usable_rows X))
  for s = 0 .. sets-1:  l_active * ( z_s(wX) * prod_{j in set s} (v_j + beta*sigma_j + gamma)
                                     - z_s * prod_{j in set s} (v_j + beta*delta^j*X_i + gamma) )
  (j runs over all eight columns across the sets; the last set may be short)

Lookup terms, T = 5 (plonk/lookup/prover.rs), columns A, S, A', S', z:

  l_0 * (1 - z)
  l_last * (z^2 - z)
  l_active * ( z(wX) * (A' + beta) * (S' + gamma) - z * (A + beta) * (S + gamma) )
  l_0 * (A' - S')
  l_active * (A' - S') * (A' - A'(w^-1 X))

The fold: h = h_in (zero when absent), then h = h*y + e_t for each term in order, so
h_out = y^T * h_in + sum_t y^(T-1-t) * e_t. The divide: h_out[i] = h_in[i] * (X_i^n - 1)^-1.

halo2 itself is not available to the tests, so parity with it is pinned by the arguments' own
property (tests/test_quotient_ref.py): for a valid argument the quotient has the degree the
vanishing division leaves, and a broken one does not."""
import ntt_ref as nr

N_PERM = 8


def selectors(k, usable_rows):
    """(l_0, l_last, l_active) in the Lagrange basis, 2^k rows each."""
    n = 1 << k
    assert 0 <= usable_rows < n
    return ([int(i == 0) for i in range(n)], [int(i == usable_rows) for i in range(n)],
            [int(i < usable_rows) for i in range(n)])


def points(ext_k, omega_ext, shift, p, rows=None):
    """X_i = shift * omega_ext^i for the rows asked (all by default)."""
    rows = range(1 << ext_k) if rows is None else rows
    return [shift * pow(omega_ext, i, p) % p for i in rows]


def extend(col, k, ext_k, omega, omega_ext, shift, p):
    """A Lagrange-form column of 2^k values on the extended coset (2^ext_k values)."""
    return nr.forward(nr.inverse(list(col), k, omega, 1, p), ext_k, omega_ext, shift, p)


def permutation_terms(k, ext_k, usable_rows, l, v, sigma, z, chunk_len, omega_ext, shift, delta, beta,
                      gamma, p, rows=None):
    """terms[t][r] for the extended rows `rows` (all by default). l = (l_0, l_last, l_active),
    v and sigma eight columns each (v_j = the permutation's column j), z the sets columns."""
    n_ext, rot = 1 << ext_k, 1 << (ext_k - k)
    sets = -(-N_PERM // chunk_len)
    assert len(v) == N_PERM and len(sigma) == N_PERM and len(z) == sets
    rows = range(n_ext) if rows is None else rows
    l0, llast, lact = l
    out = [[] for _ in range(2 * sets + 1)]
    for i in rows:
        x = shift * pow(omega_ext, i, p) % p
        nxt, link = (i + rot) % n_ext, (i + usable_rows * rot) % n_ext
        t = [l0[i] * (1 - z[0][i]) % p,
             llast[i] * (z[sets - 1][i] * z[sets - 1][i] - z[sets - 1][i]) % p]
        for s in range(1, sets):
            t.append(l0[i] * (z[s][i] - z[s - 1][link]) % p)
        for s in range(sets):
            left, right = z[s][nxt], z[s][i]
            for j in range(s * chunk_len, min((s + 1) * chunk_len, N_PERM)):
                left = left * (v[j][i] + beta * sigma[j][i] + gamma) % p
                right = right * (v[j][i] + beta * pow(delta, j, p) * x + gamma) % p
            t.append(lact[i] * (left - right) % p)
        for e, val in zip(out, t):
            e.append(val)
    return out


def lookup_terms(k, ext_k, l, cols, beta, gamma, p, rows=None):
    """terms[t][r]; cols = (A, S, A', S', z) extended."""
    n_ext, rot = 1 << ext_k, 1 << (ext_k - k)
    rows = range(n_ext) if rows is None else rows
    l0, llast, lact = l
    a, s, ap, sp, z = cols
    out = [[] for _ in range(5)]
    for i in rows:
        nxt, prv = (i + rot) % n_ext, (i - rot) % n_ext
        t = [l0[i] * (1 - z[i]) % p,
             llast[i] * (z[i] * z[i] - z[i]) % p,
             lact[i] * (z[nxt] * (ap[i] + beta) * (sp[i] + gamma) - z[i] * (a[i] + beta) * (s[i] + gamma)) % p,
             l0[i] * (ap[i] - sp[i]) % p,
             lact[i] * (ap[i] - sp[i]) * (ap[i] - ap[prv]) % p]
        for e, val in zip(out, t):
            e.append(val)
    return out


def fold(terms, y, p, h_in=None):
    """h[r] = y^T h_in[r] + sum_t y^(T-1-t) terms[t][r]."""
    count = len(terms[0])
    h = [0] * count if h_in is None else [int(x) % p for x in h_in]
    assert len(h) == count
    for e in terms:
        h = [(a * y + b) % p for a, b in zip(h, e)]
    return h


def divide(h, k, ext_k, omega_ext, shift, p, rows=None):
    """h[r] * (X_i^n - 1)^-1, i the extended row of entry r (rows; all by default)."""
    rows = range(1 << ext_k) if rows is None else rows
    out = []
    for val, i in zip(h, rows):
        d = (pow(shift * pow(omega_ext, i, p) % p, 1 << k, p) - 1) % p
        assert d, "X^n = 1 at row %d" % i
        out.append(val * pow(d, p - 2, p) % p)
    return out
