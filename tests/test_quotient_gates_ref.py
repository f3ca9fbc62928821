"""tests/quotient_gates_ref.py pinned on the CPU, two ways.

The trace is the oracle's: two instances with rounds (1, 0), 644 + 228 = 872 rows, k = 10. Its u32
cells become field integers, the fixed column its seventeen field columns, and every advice row
past the instances is filled with random elements: no gate reads them under an enabled selector,
so everything below must hold all the same.

  domain points  ext_k = k + 1 and shift = 1: the even extended rows are the 2^k domain points (the
                 extension of a column takes its own values there; checked through
                 tests/ntt_ref.py on the clean trace). A clean trace gives zero at every even row
                 for every term. For each gate bit g, a trace with one cell that gate reads altered
                 gives, for every bit, as many even rows with a non-zero term of that bit as the
                 oracle's gate_failures counts for the same trace: the term list against the
                 oracle's independent C gate code.
  degree         ext_k = k + 2 and shift = zeta: extend (tests/ntt_ref.py), fold, divide,
                 interpolate. The gates have degree <= 4 with their selector, so the numerator of
                 a satisfied trace is a multiple of X^n - 1 and the quotient has no coefficient of
                 index >= 3n - 3; with one altered cell in an enabled row of any of the 16 gates it
                 has some. One field only (pallas): the integers are what is under test, the
                 Montgomery form is a matter of packing, and a second field doubles a slow test.
"""
import numpy as np
import pytest

import ntt_ref as nr
import quotient_gates_ref as gr

from conftest import random_inputs

K = 10
N = 1 << K
FORM = 1
P = nr.modulus(FORM)

# per gate bit: a cell (a_c, rotation j) the gate reads; altered at the first row where it is on
TAMPER = {0: (7, 0), 1: (8, 3), 2: (7, 2), 3: (9, 0), 4: (0, 1), 5: (9, 0), 6: (3, 2), 7: (1, 3),
          8: (6, 2), 9: (4, 1), 10: (4, 4), 11: (8, 0), 12: (2, 7), 13: (5, 6), 14: (1, 0), 15: (5, 0)}


def _field():
    from b2f import field

    f = field.of_form(FORM)
    return field, f, pow(field.GENERATOR[f], (P - 1) // 3, P)


class Trace:
    def __init__(self, orc):
        x = random_inputs(2, (0,), 61)
        x["rounds"] = np.asarray([1, 0], dtype=np.uint32)
        ox = np.frombuffer(x.tobytes(), dtype=orc.INPUT_DTYPE).copy()
        self.adv, self.fixed, _, self.off = orc.fill(ox)
        self.used = int(self.off[-1])
        assert self.used == 872 and self.adv.shape == (10, 872)
        rng = np.random.default_rng(11)
        self.tail = [nr.random_elements(rng, N - self.used, P) for _ in range(10)]
        self.fixed_cols = [c + [0] * (N - self.used) for c in gr.unpack_fixed(self.fixed)]
        self.orc = orc

    def columns(self, adv=None):
        """The ten advice columns over 2^k rows in halo2 order (ints)."""
        adv = self.adv if adv is None else adv
        cols = [None] * 10
        for c in range(10):
            cols[gr.HALO2[c]] = [int(v) for v in adv[c]] + self.tail[c]
        return cols

    def tampered(self, g):
        """(advice with the gate's cell + 1, the halo2 column and row of the cell)."""
        c, j = TAMPER[g]
        row = int(np.flatnonzero((self.fixed >> g) & 1)[0]) + j
        adv = self.adv.copy()
        assert adv[c, row] < 2**32 - 1
        adv[c, row] += 1
        return adv, gr.HALO2[c], row

    def failures(self, adv):
        return self.orc.evaluate(adv, self.fixed, self.off)["gate_failures"]


@pytest.fixture(scope="module")
def trace(orc):
    return Trace(orc)


class Spread:
    """A 2^k column seen at the even rows of the extension by 2 with shift 1."""

    def __init__(self, col):
        self.col = col

    def __getitem__(self, i):
        assert not i & 1
        return self.col[i >> 1]


def _domain_counts(trace, adv_cols):
    """Per gate bit: the number of domain points (even extended rows) with a non-zero term."""
    terms = gr.gate_terms(K, K + 1, [Spread(c) for c in adv_cols], [Spread(c) for c in trace.fixed_cols], P,
                          rows=range(0, 2 * N, 2))
    assert len(terms) == 74 and all(len(t) == N for t in terms)
    bad = [set() for _ in range(16)]
    for t, col in enumerate(terms):
        bad[gr.TERM_GATE[t]].update(i for i, v in enumerate(col) if v)
    return [len(b) for b in bad]


def test_the_term_list_has_the_counts_of_the_layout_table():
    assert gr.N_TERMS == 74 and len(gr.TERM_GATE) == 74
    assert gr.GATE_COUNTS == (2, 8, 8, 2, 12, 2, 4, 2, 12, 2, 4, 2, 4, 4, 1, 5)
    assert gr.GATES[3] is gr.GATES[7] and gr.GATES[5] is gr.GATES[9]
    assert gr.GATES[6] is gr.GATES[10] is gr.GATES[12]


def test_even_rows_of_the_extension_by_two_are_the_domain_points(trace):
    field, f, _ = _field()
    import quotient_ref as qr

    col = trace.columns()[gr.HALO2[2]]
    ext = qr.extend(col, K, K + 1, field.omega(f, K), field.omega(f, K + 1), 1, P)
    assert ext[0::2] == col
    assert ext[1::2] != col


def test_clean_trace_vanishes_on_the_domain_and_every_gate_is_enabled_somewhere(trace):
    assert trace.failures(trace.adv) == [0] * 16
    assert _domain_counts(trace, trace.columns()) == [0] * 16
    assert all(int(((trace.fixed >> g) & 1).sum()) > 0 for g in range(16))


@pytest.mark.parametrize("g", range(16))
def test_a_tampered_cell_fails_the_terms_the_oracle_fails(trace, g):
    adv, _, _ = trace.tampered(g)
    want = trace.failures(adv)
    assert want[g] > 0
    assert _domain_counts(trace, trace.columns(adv)) == want


class Degree:
    """The clean trace on the coset at ext_k = k + 2, and the quotient's high coefficients."""

    def __init__(self, trace):
        import quotient_ref as qr

        field, f, zeta = _field()
        self.trace, self.qr = trace, qr
        self.ext_k = K + 2
        self.omega, self.omega_ext, self.shift = field.omega(f, K), field.omega(f, self.ext_k), zeta
        self.y = nr.random_elements(np.random.default_rng(12), 1, P)[0]
        self.adv = [self.extend(c) for c in trace.columns()]
        self.fixed = [self.extend(c) for c in trace.fixed_cols]

    def extend(self, col):
        return self.qr.extend(col, K, self.ext_k, self.omega, self.omega_ext, self.shift, P)

    def high_coefficients(self, adv):
        terms = gr.gate_terms(K, self.ext_k, adv, self.fixed, P)
        h = gr.divide(gr.fold(terms, self.y, P), K, self.ext_k, self.omega_ext, self.shift, P)
        return nr.inverse(h, self.ext_k, self.omega_ext, self.shift, P)[3 * N - 3:]


@pytest.fixture(scope="module")
def degree(trace):
    return Degree(trace)


def test_clean_trace_quotient_has_the_low_degree(degree):
    terms = gr.gate_terms(K, degree.ext_k, degree.adv, degree.fixed, P, rows=[1, 2, 3])
    assert any(any(t) for t in terms)  # off the domain the terms are not zero
    assert not any(degree.high_coefficients(degree.adv))


@pytest.mark.parametrize("g", range(16))
def test_one_tampered_cell_per_gate_is_no_multiple_of_the_vanishing_polynomial(trace, degree, g):
    adv, col, _ = trace.tampered(g)
    cols = list(degree.adv)
    cols[col] = degree.extend(trace.columns(adv)[col])  # the one column that changed
    assert any(degree.high_coefficients(cols))


def test_sampled_rows_equal_the_full_evaluation(degree):
    rows = [0, 1, 4095, 4052, 2048]
    full = gr.gate_terms(K, degree.ext_k, degree.adv, degree.fixed, P)
    assert gr.gate_terms(K, degree.ext_k, degree.adv, degree.fixed, P, rows=rows) == \
        [[t[i] for i in rows] for t in full]


def test_rotations_wrap_by_a_true_mod_on_small_domains():
    """k = 2, ext_k = 5: 11 rot = 88 > n_ext = 32, so a rotation wraps more than once."""
    rng = np.random.default_rng(13)
    adv = [nr.random_elements(rng, 32, P) for _ in range(10)]
    fixed = [nr.random_elements(rng, 32, P) for _ in range(17)]
    terms = gr.gate_terms(2, 5, adv, fixed, P)
    i = 30  # bit 1's last polynomial at k = 3: a_8@9 - a_2@1 - 2^16 a_2@3
    a8, a2 = adv[gr.HALO2[8]], adv[gr.HALO2[2]]
    want = fixed[1][i] * (a8[(i + 72) % 32] - a2[(i + 8) % 32] - 2**16 * a2[(i + 24) % 32]) % P
    assert terms[2 + 7][i] == want


def test_the_binding_declares_the_two_calls():
    import b2f
    from b2f import _lib

    names = {n for n, _, _ in _lib.SIGNATURES}
    assert {"b2f_export_fixed_fp_dev", "b2f_quotient_gates_dev"} <= names
    assert _lib.NUM_FIXED_FP == 17 and len(_lib.KERNEL_NAMES) == 10
    for name in ("export_fixed_fp_dev", "quotient_gates_dev", "quotient_gates"):
        assert callable(getattr(b2f.Engine, name)), name
    assert callable(b2f.DeviceBatch.export_fixed_fp)
