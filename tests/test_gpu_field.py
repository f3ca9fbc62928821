"""The device field primitives of csrc/b2f_field.h and csrc/b2f_mont_asm.h, one at a time,
against Python integers (R = 2^256), bit for bit, through the diagnostics library's
b2f_debug_field_op (csrc/b2f_fieldprobe.hip: one lane per element, operands used as given).

  1  the edge set E x E (tests/field_cases.py) through mul (the generated asm block the kernels
     call), mul_comba, mul_cios, add and sub;
  2  products crafted to have a chosen Montgomery reduction word m_k in {0, 1, 2^31, 2^32 - 2,
     2^32 - 1} at each column k (a random product takes those paths with probability 2^-31);
  3  from_u32 on every x <= 2^16, 2^j and 2^j +- 1, random x;
  4  to_mont, to_canonical on E and random elements;
  5  fe_pow on E with exponents at the word's edges;
  6  inv (binary Euclid), inv_kaliski, inv_safegcd, inv_fermat on E without 0 and random elements;
  7  the probe refuses (B2F_ERR_ARG, nothing launched) an operand >= p and a zero handed to any
     inverse: inv<F> does not terminate on 0 or on p, so no test passes either to the device.

Needs an MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

ERR_ARG = 1
FIELDS = [0, 1]  # pallas Fp, BN254 Fr
PRODUCTS = ("mul", "mul_comba", "mul_cios")
INVERSES = ("inv", "inv_kaliski", "inv_safegcd", "inv_fermat")


def _op(eng, op, field, a, b=None):
    """Run `op` on int operands; returns (results as ints, flags)."""
    b = [0] * len(a) if b is None else b
    out, flags = eng.debug_field_op(op, fc.pack(a), fc.pack(b), field)
    return fc.unpack(out), flags


def _first_bad(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i
    return None


def _check(eng, op, field, a, b, want):
    got, flags = _op(eng, op, field, a, b)
    bad = _first_bad(got, want)
    assert bad is None, "%s field %d element %d: a=%#x b=%#x got %#x want %#x" % (
        op, field, bad, a[bad], (b or [0] * len(a))[bad], got[bad], want[bad])
    assert (flags == 1).all(), (op, field, int(np.flatnonzero(flags != 1)[0]))
    return got


@pytest.mark.parametrize("field", FIELDS)
def test_edge_pairs_products_add_sub(diag_engine, field):
    p = fc.MODULI[field]
    rinv = pow(fc.R, -1, p)
    pairs = fc.edge_pairs(p)
    assert len(pairs) == 17 * 17
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    want = [x * y * rinv % p for x, y in pairs]
    got = [_check(diag_engine, op, field, a, b, want) for op in PRODUCTS]
    assert got[0] == got[1] == got[2]
    _check(diag_engine, "add", field, a, b, [(x + y) % p for x, y in pairs])
    _check(diag_engine, "sub", field, a, b, [(x - y) % p for x, y in pairs])


@pytest.mark.parametrize("field", FIELDS)
def test_crafted_reduction_words(diag_engine, field):
    p = fc.MODULI[field]
    rinv = pow(fc.R, -1, p)
    crafted = fc.crafted_pairs(p)  # asserts a b (-p^-1) mod R == m, word k of m == v
    print("field %d: %d of %d crafted targets built" % (field, len(crafted), fc.CRAFT_TARGETS))
    assert len(crafted) >= fc.CRAFT_MIN_FOUND, (len(crafted), fc.CRAFT_TARGETS)
    # every (column, word) has a pair of some filling; a result in [p, 2p) before the last
    # subtraction is among them
    assert {(k, v) for k, v, _, _, _ in crafted} == {(k, v) for k in range(8) for v in fc.CRAFT_WORDS}
    a, b = [c[3] for c in crafted], [c[4] for c in crafted]
    assert any((x * y + (x * y * pow(fc.R - p, -1, fc.R) % fc.R) * p) >> 256 >= p for x, y in zip(a, b))
    want = [x * y * rinv % p for x, y in zip(a, b)]
    got = [_check(diag_engine, op, field, a, b, want) for op in PRODUCTS]
    assert got[0] == got[1] == got[2]
    # the product is symmetric in value, not in code: b's words walk the other index
    for op in PRODUCTS:
        _check(diag_engine, op, field, b, a, want)


@pytest.mark.parametrize("field", FIELDS)
def test_crafted_column_carry(diag_engine, field):
    """A column whose high word is 2^32 - 1 when its low word cancels: the carry runs through the
    whole word into the carry word (pallas: the borrow of m_k = 0 - ACC.lo added to ACC.hi)."""
    p = fc.MODULI[field]
    rinv = pow(fc.R, -1, p)
    carry = fc.carry_pairs(p)
    print("field %d: %d of %d column-carry targets built" % (field, len(carry), fc.CARRY_TARGETS))
    assert len(carry) >= fc.CARRY_MIN_FOUND, (len(carry), fc.CARRY_TARGETS)
    assert {k for k, _, _ in carry} == set(range(1, 8))
    for k, x, y in carry:
        v = fc.column_sum(p, x, y, k)
        assert (v >> 32) & fc.M32 == fc.M32 and v & fc.M32
    a, b = [c[1] for c in carry], [c[2] for c in carry]
    want = [x * y * rinv % p for x, y in zip(a, b)]
    got = [_check(diag_engine, op, field, a, b, want) for op in PRODUCTS]
    assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("field", FIELDS)
def test_from_u32(diag_engine, field):
    p = fc.MODULI[field]
    rng = random.Random(21 + field)
    xs = list(range(0, (1 << 16) + 1))
    for j in range(33):
        xs += [v for v in ((1 << j) - 1, 1 << j, (1 << j) + 1) if 0 <= v < 1 << 32]
    xs.append((1 << 32) - 1)
    xs += [rng.getrandbits(32) for _ in range(4096)]
    # the probe takes at most 65,536 elements a call
    for lo in range(0, len(xs), 65536):
        part = xs[lo:lo + 65536]
        _check(diag_engine, "from_u32", field, part, None, [x * fc.R % p for x in part])


@pytest.mark.parametrize("field", FIELDS)
def test_to_mont_to_canonical(diag_engine, field):
    p = fc.MODULI[field]
    rng = random.Random(31 + field)
    rinv = pow(fc.R, -1, p)
    xs = fc.edge_set(p) + [rng.randrange(p) for _ in range(1024)]
    _check(diag_engine, "to_mont", field, xs, None, [x * fc.R % p for x in xs])
    _check(diag_engine, "to_canonical", field, xs, None, [x * rinv % p for x in xs])


@pytest.mark.parametrize("field", FIELDS)
def test_fe_pow(diag_engine, field):
    p = fc.MODULI[field]
    rinv = pow(fc.R, -1, p)
    exps = (0, 1, 2, 3, 1 << 16, 1 << 31, (1 << 32) - 1)
    a = [x for x in fc.edge_set(p) for _ in exps]
    e = [y for _ in fc.edge_set(p) for y in exps]
    # Montgomery form in, Montgomery form out; x^0 = 1 for x = 0 too
    want = [pow(x * rinv % p, y, p) * fc.R % p for x, y in zip(a, e)]
    _check(diag_engine, "fe_pow", field, a, e, want)


@pytest.mark.parametrize("field", FIELDS)
def test_inverses(diag_engine, field):
    p = fc.MODULI[field]
    rng = random.Random(41 + field)
    rinv = pow(fc.R, -1, p)
    xs = [x for x in fc.edge_set(p) if x] + [rng.randrange(1, p) for _ in range(512)]
    assert all(0 < x < p for x in xs)  # inv<F> does not terminate on 0
    want = [pow(x * rinv % p, -1, p) * fc.R % p for x in xs]
    got = [_check(diag_engine, op, field, xs, None, want) for op in INVERSES]  # flag 1: safegcd's ok
    assert got[0] == got[1] == got[2] == got[3]


@pytest.mark.parametrize("field", FIELDS)
def test_probe_refuses_operands_the_device_cannot_take(diag_engine, field):
    from b2f import B2FError, _lib

    p = fc.MODULI[field]
    for op in _lib.FIELD_OPS:
        for a, b in ((p, 1), (1, p), (p + 1, 1), (2**256 - 1, 1), (1, 2**256 - 1)):
            with pytest.raises(B2FError) as e:
                _op(diag_engine, op, field, [1, a], [1, b])
            assert e.value.code == ERR_ARG, (op, hex(a), hex(b))
    for op in INVERSES:
        with pytest.raises(B2FError) as e:
            _op(diag_engine, op, field, [1, 0, 2])
        assert e.value.code == ERR_ARG, op
    lib = diag_engine.lib
    one = fc.pack([1])
    out, flags = np.zeros((1, 4), np.uint64), np.zeros(1, np.uint32)
    ptr = lambda x: x.ctypes.data  # noqa: E731
    assert lib.b2f_debug_field_op(field, len(_lib.FIELD_OPS), ptr(one), ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_field_op(2, 0, ptr(one), ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_field_op(field, 0, ptr(one), ptr(one), 65537, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_field_op(field, 0, ptr(one), ptr(one), 0, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_field_op(field, 0, None, ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    # a good call after the refusals
    _check(diag_engine, "add", field, [p - 1], [1], [0])
