"""Big-integer restatement (Python ints) of b2f_quotient_gates_dev (include/b2f.h): the 74
custom-gate terms of the BLAKE2f chip on the extended coset, straight from the table of
docs/LAYOUT.md §4, in the order of docs/LAYOUT.md §4.1. It depends on tests/quotient_ref.py only
(whose `fold` and `divide` it reuses).

n = 2^k, n_ext = 2^ext_k, rot = 2^(ext_k - k); cell x@j of extended row i is row
(i + j * rot) mod n_ext of column x. `adv` holds the ten advice columns in halo2's order (the block
b2f_export_fp_dev writes: a_i is column HALO2[i]); `fixed` the seventeen fixed columns of
b2f_export_fixed_fp_dev (selector bit g is column g, k_0 column 16). A column is anything
indexable by the extended row. Each term is q_g * p with q_g = fixed[g] at the row itself.

halo2 itself is not available to the tests: tests/test_quotient_gates_ref.py pins this file to the
oracle's independent gate code on the 2^k domain, and by the degree of the quotient."""
from quotient_ref import divide, fold  # noqa: F401  (re-exported for the tests)

HALO2 = (7, 8, 9, 1, 2, 0, 3, 4, 5, 6)  # halo2 column of a_i (b2f_halo2_column_index)
GATE_COUNTS = (2, 8, 8, 2, 12, 2, 4, 2, 12, 2, 4, 2, 4, 4, 1, 5)
N_TERMS = sum(GATE_COUNTS)  # 74
TERM_GATE = tuple(g for g, m in enumerate(GATE_COUNTS) for _ in range(m))
N_FIXED = 17


def _decompose_abcd(a):
    return [a(7, 0) - a(1, 0) - 2**16 * a(1, 1), a(8, 0) - a(1, 2) - 2**16 * a(1, 3)]


def _decompose_efgh(a):
    out = []
    for k in range(4):
        k1, k2 = (k + 1) & 3, (k + 2) & 3
        out += [a(7, 3 * k) - a(1, 3 * k1 + 1) - 2**8 * a(1, 3 * k2),
                a(8, 3 * k) - a(2, 3 * k1 + 1) - 2**16 * a(2, 3 * k2)]
    return out


def _decompose_ijkl(a):
    out = []
    for k in range(4):
        k3 = (k + 3) & 3
        out += [a(7, 2 * k) - a(6, 2 * k3) - 2 * a(1, 2 * k),
                a(8, 2 * k) - a(6, 2 * k3) - 4 * a(2, 2 * k)]
    return out


def _add3(a):
    c = a(9, 0)
    return [sum(2**(16 * k) * (a(3, k) + a(4, k) + a(5, k) - a(1, k)) for k in range(4)) - 2**64 * c,
            c * (c - 1) * (c - 2)]


def _add2(a):
    c = a(9, 0)
    return [sum(2**(16 * k) * (a(3, k) + a(4, k) - a(1, k)) for k in range(4)) - 2**64 * c,
            c * (c - 1)]


def _xor24(a):
    out = []
    for k in range(4):
        out += [a(3, 3 * k) + a(4, 3 * k) - a(2, 3 * k) - 2**16 * a(2, 3 * k + 1) - 2 * a(2, 3 * k + 2),
                a(0, 3 * k), a(0, 3 * k + 1)]
    return out


def _xor(a):
    return [a(3, 2 * k) + a(4, 2 * k) - a(2, 2 * k) - 2 * a(2, 2 * k + 1) for k in range(4)]


def _xor63(a):
    out = []
    for k in range(4):
        out += [a(3, 2 * k) + a(4, 2 * k) - a(2, 2 * k) - 2**30 * a(6, 2 * k) - 2 * a(2, 2 * k + 1),
                a(0, 2 * k) * (a(0, 2 * k) - 1), a(6, 2 * k) * (a(6, 2 * k) - 1)]
    return out


def _digest(a):
    return [a(7, 0) - a(1, 0) - 2**16 * a(1, 2), a(8, 0) - a(1, 4) - 2**16 * a(1, 6)]


def _xor3(a):
    return [a(3, 2 * k) + a(4, 2 * k) + a(5, 2 * k) - a(2, 2 * k) - 2 * a(2, 2 * k + 1) for k in range(4)]


def _fmask(a):
    return [a(5, 0) * (a(5, 0) - 1)] + [a(1, k) - 65535 * a(5, 0) for k in range(4)]


# selector bit -> the polynomials of its cell in the LAYOUT.md §4 table (bit 14 apart: it reads k_0)
GATES = {0: _decompose_abcd, 1: _decompose_efgh, 2: _decompose_ijkl, 3: _add3, 4: _xor24, 5: _add2,
         6: _xor, 7: _add3, 8: _xor63, 9: _add2, 10: _xor, 11: _digest, 12: _xor, 13: _xor3, 15: _fmask}


def gate_terms(k, ext_k, adv, fixed, p, rows=None):
    """terms[t][r] for the extended rows `rows` (all by default), t = 0..73 in the call's order."""
    n_ext, rot = 1 << ext_k, 1 << (ext_k - k)
    assert len(adv) == 10 and len(fixed) == N_FIXED
    rows = range(n_ext) if rows is None else rows
    out = [[] for _ in range(N_TERMS)]
    for i in rows:
        def a(c, j):
            return adv[HALO2[c]][(i + j * rot) % n_ext]

        t = 0
        for g in range(16):
            polys = [a(1, 0) - fixed[16][i]] if g == 14 else GATES[g](a)
            assert len(polys) == GATE_COUNTS[g]
            q = fixed[g][i]
            for poly in polys:
                out[t].append(q * poly % p)
                t += 1
    return out


def unpack_fixed(q):
    """The packed fixed column (mask | k_0 << 16 per row) as the seventeen columns of ints."""
    q = [int(v) for v in q]
    return [[(v >> g) & 1 for v in q] for g in range(16)] + [[v >> 16 for v in q]]
