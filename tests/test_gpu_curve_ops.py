"""The device base-field primitives and point operations of the commitment curves
(csrc/b2f_field.h on VestaBase / Bn254Base, csrc/b2f_curve.h), one per lane through the
diagnostics library's b2f_debug_curve_op (csrc/b2f_curveprobe.hip), bit for bit against Python
integers (tests/msm_ref.py). Point results are compared as affine points.

  1  mul, add, sub on the edge set E x E, the crafted reduction words, the column carries and
     random pairs; to_mont, to_canonical on E and random elements; inv_safegcd on E and random
     elements (0 gives 0);
  2  madd (XYZZ accumulator + affine), padd (XYZZ + XYZZ), dbl, mdbl, neg on random points with
     random z (accumulators that are not normalised);
  3  every degenerate pairing, mixed and full: identity + P, P + identity, identity + identity,
     P + P (falls through to the doubling), P + (-P) (the identity), doubling the identity, and the
     same with differently scaled representations of equal / opposite points;
  4  the probe refuses an operand >= q, an unknown curve or op, n = 0.

Needs an MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import field_cases as fc
import msm_ref as mr

pytestmark = pytest.mark.gpu

CURVES = [0, 1]
ERR_ARG = 1


def _fop(eng, op, cv, a, b=None):
    b = [0] * len(a) if b is None else b
    out, flags = eng.debug_curve_op(op, fc.pack(a), fc.pack(b), cv)
    return fc.unpack(out), flags


def _fcheck(eng, op, cv, a, b, want):
    got, flags = _fop(eng, op, cv, a, b)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s curve %d element %d: a=%#x b=%#x got %#x want %#x" % (
            op, cv, i, a[i], (b or [0] * len(a))[i], g, w)
    assert (flags == 1).all(), (op, cv)


@pytest.mark.parametrize("cv", CURVES)
def test_base_field_mul_add_sub(diag_engine, cv):
    q = mr.Q[cv]
    rinv = pow(fc.R, -1, q)
    rng = random.Random(60 + cv)
    crafted = fc.crafted_pairs(q)
    carry = fc.carry_pairs(q)
    print("curve %d: crafted %d / %d, carry %d / %d" % (cv, len(crafted), fc.CRAFT_TARGETS, len(carry),
                                                       fc.CARRY_TARGETS))
    assert len(crafted) >= fc.CRAFT_MIN_FOUND and len(carry) >= fc.CARRY_MIN_FOUND
    pairs = fc.edge_pairs(q) + [(c[3], c[4]) for c in crafted] + [(c[4], c[3]) for c in crafted]
    pairs += [(c[1], c[2]) for c in carry] + [(rng.randrange(q), rng.randrange(q)) for _ in range(300)]
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    _fcheck(diag_engine, "mul", cv, a, b, [x * y * rinv % q for x, y in pairs])
    _fcheck(diag_engine, "add", cv, a, b, [(x + y) % q for x, y in pairs])
    _fcheck(diag_engine, "sub", cv, a, b, [(x - y) % q for x, y in pairs])


@pytest.mark.parametrize("cv", CURVES)
def test_base_field_forms_and_inverse(diag_engine, cv):
    q = mr.Q[cv]
    rinv = pow(fc.R, -1, q)
    rng = random.Random(61 + cv)
    xs = fc.edge_set(q) + [rng.randrange(q) for _ in range(512)]
    _fcheck(diag_engine, "to_mont", cv, xs, None, [x * fc.R % q for x in xs])
    _fcheck(diag_engine, "to_canonical", cv, xs, None, [x * rinv % q for x in xs])
    # Montgomery form in and out; 0 gives 0 with ok set
    want = [pow(x * rinv % q, -1, q) * fc.R % q if x else 0 for x in xs]
    _fcheck(diag_engine, "inv_safegcd", cv, xs, None, want)


def _pop(eng, op, cv, a, b, za, zb):
    """Point op on affine int points (None: identity), lifted with the ints za, zb (canonical)."""
    q = mr.Q[cv]
    out, flags = eng.debug_curve_op(op, mr.pack_points(cv, a), mr.pack_points(cv, b), cv,
                                    fc.pack([z * fc.R % q for z in za]), fc.pack([z * fc.R % q for z in zb]))
    assert (flags == 1).all(), (op, cv)
    return mr.unpack_points(cv, out)


def _pcheck(eng, op, cv, a, b, za, zb, want, label=""):
    got = _pop(eng, op, cv, a, b, za, zb)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s curve %d %s element %d: a=%s b=%s za=%#x zb=%#x" % (op, cv, label, i, a[i], b[i],
                                                                               za[i], zb[i])


@pytest.mark.parametrize("cv", CURVES)
def test_point_ops_on_random_points(diag_engine, cv):
    q = mr.Q[cv]
    rng = random.Random(70 + cv)
    _, pool = mr.known_bases(2 * cv, 256)
    a, b = pool[:128], pool[128:256]
    za = [1, q - 1, 2] + [rng.randrange(1, q) for _ in range(125)]
    zb = [rng.randrange(1, q) for _ in range(126)] + [1, q - 1]
    sums = [mr.add(cv, x, y) for x, y in zip(a, b)]
    _pcheck(diag_engine, "madd", cv, a, b, za, zb, sums)
    _pcheck(diag_engine, "padd", cv, a, b, za, zb, sums)
    dbls = [mr.double(cv, x) for x in a]
    _pcheck(diag_engine, "dbl", cv, a, b, za, zb, dbls)
    _pcheck(diag_engine, "mdbl", cv, a, b, za, zb, dbls)
    _pcheck(diag_engine, "neg", cv, a, b, za, zb, [mr.neg(cv, x) for x in a])


@pytest.mark.parametrize("cv", CURVES)
def test_degenerate_pairings(diag_engine, cv):
    q = mr.Q[cv]
    rng = random.Random(80 + cv)
    _, pool = mr.known_bases(2 * cv, 8)
    g = mr.GEN[cv]
    a, b, za, zb, want = [], [], [], [], []

    def case(x, y, zx, zy):
        a.append(x)
        b.append(y)
        za.append(zx)
        zb.append(zy)
        want.append(mr.add(cv, x if zx else None, y if zy else None))

    for p in [g] + pool:
        for zx in (1, q - 1, rng.randrange(2, q)):
            for zy in (1, rng.randrange(2, q)):
                case(None, p, zx, zy)            # identity + P
                case(p, None, zx, zy)            # P + identity
                case(p, p, zx, zy)               # equal points: the doubling
                case(p, mr.neg(cv, p), zx, zy)   # opposite points: the identity
                case(mr.neg(cv, p), p, zx, zy)
        case(p, p, 0, 1)                         # z = 0 makes the accumulator the identity
    case(None, None, 1, 1)
    case(None, None, 0, 0)
    assert any(w is None for w in want) and any(w is not None for w in want)
    _pcheck(diag_engine, "padd", cv, a, b, za, zb, want, "degenerate")
    # madd's addend is affine: zb does not apply
    want_m = [mr.add(cv, x if zx else None, y) for x, y, zx in zip(a, b, za)]
    _pcheck(diag_engine, "madd", cv, a, b, za, zb, want_m, "degenerate")
    # doubling: of the identity, and of lifted points
    want_d = [mr.double(cv, x if zx else None) for x, zx in zip(a, za)]
    _pcheck(diag_engine, "dbl", cv, a, b, za, zb, want_d, "degenerate")
    _pcheck(diag_engine, "mdbl", cv, a, b, za, zb, [mr.double(cv, x) for x in a], "degenerate")
    _pcheck(diag_engine, "neg", cv, a, b, za, zb, [mr.neg(cv, x if zx else None) for x, zx in zip(a, za)],
            "degenerate")


@pytest.mark.parametrize("cv", CURVES)
def test_probe_refusals(diag_engine, cv):
    from b2f import B2FError, _lib

    q = mr.Q[cv]
    for op in ("mul", "add", "inv_safegcd"):
        for x, y in ((q, 1), (1, q), (2**256 - 1, 1)):
            with pytest.raises(B2FError) as e:
                _fop(diag_engine, op, cv, [1, x], [1, y])
            assert e.value.code == ERR_ARG
    g = mr.pack_points(cv, [mr.GEN[cv]])
    bad = g.copy()
    bad[0, 4:8] = fc.pack([q])[0]  # y = q
    one = fc.pack([1])
    with pytest.raises(B2FError):
        diag_engine.debug_curve_op("padd", bad, g, cv, one, one)
    with pytest.raises(B2FError):
        diag_engine.debug_curve_op("padd", g, g, cv, fc.pack([q]), one)
    lib = diag_engine.lib
    out, flags = np.zeros((1, 8), np.uint64), np.zeros(1, np.uint32)
    ptr = lambda x: x.ctypes.data  # noqa: E731
    n_ops = len(_lib.CURVE_OPS)
    assert lib.b2f_debug_curve_op(cv, n_ops, ptr(g), ptr(g), ptr(one), ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_curve_op(2, 0, ptr(g), ptr(g), ptr(one), ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_curve_op(cv, 0, ptr(g), ptr(g), ptr(one), ptr(one), 0, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_curve_op(cv, 6, ptr(g), ptr(g), None, ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    assert lib.b2f_debug_curve_op(cv, 0, None, ptr(g), ptr(one), ptr(one), 1, ptr(out), ptr(flags)) == ERR_ARG
    # a good call after the refusals
    _pcheck(diag_engine, "padd", cv, [mr.GEN[cv]], [mr.GEN[cv]], [1], [1], [mr.double(cv, mr.GEN[cv])])
