"""Big-integer reference (Python ints) of the evaluation / opening calls of include/b2f.h
(b2f_poly_eval_dev, b2f_poly_combine_dev, b2f_kate_divide_dev) and of the field side of halo2's
multiopen prover composed from them (halo2_proofs 0.3.0 arithmetic.rs eval_polynomial and
kate_division, poly/multiopen/prover.rs). It depends on tests/ntt_ref.py only.

halo2 itself is not available to the tests: tests/test_open_ref.py pins this file by its own
properties (division identities, schoolbook division, the multiopen identity)."""
from ntt_ref import pack, random_elements, unpack  # noqa: F401  (re-exported for the tests)


def eval(coeffs, z, p):  # noqa: A001  (the name of halo2's eval_polynomial)
    """sum_i coeffs[i] z^i by Horner."""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % p
    return acc


def combine(cols, terms, length, p):
    """sum of scalar * cols[c] over the (c, scalar) terms, on the first `length` rows."""
    out = [0] * length
    for c, s in terms:
        col = cols[c]
        for i in range(length):
            out[i] = (out[i] + s * col[i]) % p
    return out


def kate_division(a, z, p):
    """halo2's kate_division: the len(a) - 1 coefficients of floor(a(X) / (X - z)); the recurrence
    q_{len-1} = 0, q_{i-1} = a_i + z q_i."""
    q = [0] * (len(a) - 1)
    t = 0
    for i in range(len(a) - 1, 0, -1):
        t = (a[i] + z * t) % p
        q[i - 1] = t
    return q


def divide_chain(a, points, p):
    """kate_division for each point in turn, resized to len(a) with zeros (halo2 resizes to n);
    len(a) points or more leave nothing."""
    if len(points) >= len(a):  # more roots than coefficients: nothing is left (and no O(n^2) loop)
        return [0] * len(a)
    q = list(a)
    for z in points:
        q = kate_division(q, z, p)
    return q + [0] * (len(a) - len(q))


def kate_division_blocked(a, z, tile, p):
    """The same quotient (len(a) entries, the top one zero) by the tiled formulas of the device
    kernels: for tile t over [s, e): S_j = sum_{j < i < e} a_i z^(i-j-1), G_t = sum_{s <= i < e}
    a_i z^(i-s), carry_t = G_t + z^T carry_{t+1}, q_j = S_j + z^(e-1-j) carry_{t+1}."""
    n = len(a)
    ntiles = (n + tile - 1) // tile
    padded = list(a) + [0] * (ntiles * tile - n)
    zp = [1] * (tile + 1)
    for i in range(tile):
        zp[i + 1] = zp[i] * z % p
    g = [sum(padded[t * tile + i] * zp[i] for i in range(tile)) % p for t in range(ntiles)]
    carry = [0] * (ntiles + 1)
    zt = zp[tile]
    for t in range(ntiles - 1, -1, -1):
        carry[t] = (g[t] + zt * carry[t + 1]) % p
    q = []
    for j in range(n):
        t = j // tile
        e = (t + 1) * tile
        s_j = sum(padded[i] * zp[i - j - 1] for i in range(j + 1, e))
        q.append((s_j + zp[e - 1 - j] * carry[t + 1]) % p)
    return q, carry[0]


def poly_mul(a, b, p):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return out


def vanishing(points, p):
    """prod (X - z) over the points, lowest coefficient first."""
    out = [1]
    for z in points:
        out = poly_mul(out, [(-z) % p, 1], p)
    return out


def poly_divmod(a, d, p):
    """Schoolbook division by a monic d: (quotient, remainder)."""
    assert d[-1] == 1
    r = list(a)
    q = [0] * max(len(a) - len(d) + 1, 0)
    for i in range(len(a) - len(d), -1, -1):
        c = r[i + len(d) - 1]
        q[i] = c
        for j, dj in enumerate(d):
            r[i + j] = (r[i + j] - c * dj) % p
    return q, r[:len(d) - 1]


def interpolate(points, evals, p):
    """The polynomial of degree < len(points) through (points[i], evals[i]); distinct points."""
    out = [0] * len(points)
    for i, (xi, yi) in enumerate(zip(points, evals)):
        others = [z for j, z in enumerate(points) if j != i]
        num = vanishing(others, p)
        den = 1
        for z in others:
            den = den * (xi - z) % p
        c = yi * pow(den, p - 2, p) % p
        for j, v in enumerate(num):
            out[j] = (out[j] + c * v) % p
    return out


def multiopen_field_side(polys, sets, x1, x2, x3, x4, p):
    """The field side of halo2's multiopen prover (poly/multiopen/prover.rs create_proof). polys:
    coefficient lists of one length n; sets: (points, poly indices) pairs, every polynomial of a
    set opened at every point of it. Per set: q = sum x1-fold of its polynomials (q = q x1 + poly
    in order), the evaluations of each polynomial at each point folded the same way, r = their
    interpolation; f = x2-fold over the sets of (q - r) divided by (X - point) for each point,
    resized to n; then the q are evaluated at x3 and final = x4-fold of the q starting from f.
    Returns a dict of every intermediate."""
    n = len(polys[0])
    q_polys, q_evals, r_polys, quotients = [], [], [], []
    f = [0] * n
    for points, members in sets:
        q, ev = [0] * n, [0] * len(points)
        for m in members:
            q = [(v * x1 + c) % p for v, c in zip(q, polys[m])]
            ev = [(e * x1 + eval(polys[m], z, p)) % p for e, z in zip(ev, points)]
        r = interpolate(points, ev, p)
        diff = [(c - (r[i] if i < len(r) else 0)) % p for i, c in enumerate(q)]
        quo = divide_chain(diff, points, p)
        f = [(v * x2 + c) % p for v, c in zip(f, quo)]
        q_polys.append(q)
        q_evals.append(ev)
        r_polys.append(r)
        quotients.append(quo)
    q_at_x3 = [eval(q, x3, p) for q in q_polys]
    final = f
    for q in q_polys:
        final = [(v * x4 + c) % p for v, c in zip(final, q)]
    return {"q_polys": q_polys, "q_evals": q_evals, "r_polys": r_polys, "quotients": quotients, "f_poly": f,
            "q_at_x3": q_at_x3, "final_poly": final}
