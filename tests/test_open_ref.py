"""tests/open_ref.py pinned by its own properties (no GPU), the binding's signatures of the
evaluation / opening calls, and b2f_gate_queries against the gate polynomials of
tests/quotient_gates_ref.py."""
import re

import numpy as np
import pytest

import ntt_ref as nr
import open_ref as orf
import quotient_gates_ref as gr

FORMS = [1, 3]  # one per field


def _rand(seed, count, p):
    return nr.random_elements(np.random.default_rng(seed), count, p)


@pytest.mark.parametrize("form", FORMS)
def test_division_identity_coefficient_by_coefficient(form):
    p = nr.modulus(form)
    for n in (1, 2, 3, 17, 64):
        a = _rand(10 + n, n, p)
        a[0] = 0
        a[-1] = p - 1
        for z in (0, 1, p - 1, _rand(20 + n, 1, p)[0]):
            q = orf.kate_division(a, z, p)
            assert len(q) == n - 1
            back = orf.poly_mul(q, [(-z) % p, 1], p) if q else [0]
            back = back + [0] * (n - len(back))
            back[0] = (back[0] + orf.eval(a, z, p)) % p
            assert back == a, (n, z)


@pytest.mark.parametrize("form", FORMS)
def test_chain_is_floor_division_by_the_product(form):
    p = nr.modulus(form)
    n = 40
    a = _rand(31, n, p)
    pts = _rand(32, 5, p)
    for points in (pts[:1], pts[:3], pts, pts[::-1], [pts[0], pts[1], pts[0]], [0, 1, p - 1], [pts[2]] * 4):
        want, _ = orf.poly_divmod(a, orf.vanishing(points, p), p)
        got = orf.divide_chain(a, points, p)
        assert len(got) == n
        assert got == want + [0] * (n - len(want)), points
    assert orf.divide_chain(a, [], p) == a
    q = a[:3]
    for z in pts[:2]:
        q = orf.kate_division(q, z, p)
    assert len(q) == 1 and orf.kate_division(q, pts[2], p) == []  # a third point leaves nothing
    assert orf.divide_chain(a[:3], pts[:3], p) == [0, 0, 0]
    assert orf.divide_chain(a[:3], pts[:4], p) == [0, 0, 0]
    assert orf.divide_chain(a[:3], pts[:2], p) == [a[2], 0, 0]


@pytest.mark.parametrize("tile", [1, 3, 64])
def test_blocked_formulas_equal_the_recurrence(tile):
    form = 3
    p = nr.modulus(form)
    a_all = _rand(41, 200, p)
    zs = [0, 1, p - 1, _rand(42, 1, p)[0]]
    for n in range(1, 201):
        a = a_all[:n]
        z = zs[n % 4]
        q, carry0 = orf.kate_division_blocked(a, z, tile, p)
        assert q == orf.kate_division(a, z, p) + [0], (n, z)
        assert carry0 == orf.eval(a, z, p)


@pytest.mark.parametrize("form", FORMS)
def test_multiopen_identity_at_a_random_point(form):
    p = nr.modulus(form)
    n = 32
    polys = [_rand(50 + i, n, p) for i in range(6)]
    x, w = _rand(60, 2, p)
    sets = [([x], [0, 1, 2]), ([x, x * w % p], [3, 4]), ([x, x * w % p, x * pow(w, p - 2, p) % p], [5, 0])]
    x1, x2, x3, x4, t = _rand(61, 5, p)
    mo = orf.multiopen_field_side(polys, sets, x1, x2, x3, x4, p)
    f_at_t = 0
    for (points, members), q, ev, r, quo in zip(sets, mo["q_polys"], mo["q_evals"], mo["r_polys"],
                                                mo["quotients"]):
        assert [orf.eval(q, z, p) for z in points] == ev == [orf.eval(r, z, p) for z in points]
        assert len(quo) == n and quo[n - len(points):] == [0] * len(points)
        lhs = (orf.eval(q, t, p) - orf.eval(r, t, p)) % p
        assert lhs == orf.eval(quo, t, p) * orf.eval(orf.vanishing(points, p), t, p) % p
        f_at_t = (f_at_t * x2 + orf.eval(quo, t, p)) % p
    assert orf.eval(mo["f_poly"], t, p) == f_at_t
    want = f_at_t
    for q in mo["q_polys"]:
        want = (want * x4 + orf.eval(q, t, p)) % p
    assert orf.eval(mo["final_poly"], t, p) == want
    assert mo["q_at_x3"] == [orf.eval(q, x3, p) for q in mo["q_polys"]]


def test_combine_and_pack_roundtrip():
    p = nr.modulus(1)
    cols = [_rand(70 + i, 9, p) for i in range(3)]
    got = orf.combine(cols, [(0, 1), (2, p - 1), (0, 5)], 7, p)
    assert got == [(6 * a - c) % p for a, c in zip(cols[0][:7], cols[2][:7])]
    assert orf.combine(cols, [], 4, p) == [0] * 4
    assert orf.unpack(orf.pack(cols[1], 1), 1) == cols[1]


def _header_arity(name):
    from b2f import _lib

    with open(_lib.HEADER) as fh:
        text = fh.read()
    m = re.search(r"B2F_API\s+[\w\s\*]+?\b%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, name
    args = m.group(1).strip()
    return 0 if args == "void" else args.count(",") + 1


def test_signatures_carry_the_four_calls_with_the_headers_arity():
    from b2f import _lib

    sig = {name: args for name, _, args in _lib.SIGNATURES}
    for name in ("b2f_poly_eval_dev", "b2f_poly_combine_dev", "b2f_kate_divide_dev", "b2f_gate_queries"):
        assert name in sig, name
        assert len(sig[name]) == _header_arity(name), name
    assert len(_lib.KERNEL_NAMES) == 10


def test_gate_queries_are_the_reads_of_the_reference_gates():
    import b2f

    want = set()

    def a(c, j):
        want.add((gr.HALO2[c], j))
        return 0

    for g in sorted(gr.GATES):
        gr.GATES[g](a)
    want.add((gr.HALO2[1], 0))  # gate 14: a_1@0 - k_0
    got = [tuple(int(v) for v in row) for row in b2f.gate_queries()]
    assert got == sorted(want)
    assert all(0 <= r <= 11 for _, r in got)
    assert len(set(got)) == len(got)
    # the count-and-cap pattern of b2f_copy_constraints
    lib = b2f.load()
    few = np.full((5, 2), 0xFFFFFFFF, dtype=np.uint32)
    assert lib.b2f_gate_queries(few.ctypes.data, 3) == len(got)
    assert [tuple(int(v) for v in row) for row in few[:3]] == got[:3]
    assert (few[3:] == 0xFFFFFFFF).all()


def test_rotated_points():
    from b2f import field

    for f, form in ((field.PALLAS, 1), (field.BN254, 3)):
        p = nr.modulus(form)
        w = field.omega(f, 8)
        x = _rand(80, 1, p)[0]
        got = field.rotated_points(f, x, 8, [0, 1, -1, 11, -3])
        assert got == [x, x * w % p, x * pow(w, p - 2, p) % p, x * pow(w, 11, p) % p,
                       x * pow(w, p - 1 - 3, p) % p]
