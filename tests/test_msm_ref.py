"""CPU checks around the commitments (b2f_msm_dev): the reference's own curve constants, the naive
MSM against the known-multiple formula the GPU tests rest on, the generated base-field products
through the instruction interpreter of tests/test_mont_asm_gen.py, the base-field constants of
csrc/b2f_field.h, b2f_msm_plan (host only) and what the two libraries export."""
import os
import random
import re

import pytest

import field_cases as fc
import msm_ref as mr
from conftest import ROOT
from test_mont_asm_gen import _gen, _mont, _val

CURVES = [0, 1]


@pytest.mark.parametrize("cv", CURVES)
def test_curve_constants(cv):
    g, r = mr.GEN[cv], mr.ORDER[cv]
    assert mr.on_curve(cv, g) and g is not None
    assert not mr.on_curve(cv, (0, 0))  # the all-zero identity encoding is no curve point
    assert mr.mul(cv, r, g) is None
    assert mr.mul(cv, r - 1, g) == mr.neg(cv, g)
    assert mr.gen_mul(cv, r - 1) == mr.neg(cv, g) and mr.gen_mul(cv, 0) is None
    assert mr.add(cv, g, g) == mr.double(cv, g) == mr.mul(cv, 2, g)
    assert mr.add(cv, g, mr.neg(cv, g)) is None
    # the package's constants are the same curves
    from b2f import curve

    assert curve.BASE_MODULUS[cv] == mr.Q[cv] and curve.B[cv] == mr.B[cv]
    assert curve.ORDER[cv] == mr.ORDER[cv] and curve.GENERATOR[cv] == g
    assert curve.of_form(2 * cv) == curve.of_form(2 * cv + 1) == cv
    pts = [g, None, mr.gen_mul(cv, 12345)]
    packed = curve.pack_points(cv, pts)
    assert (packed == mr.pack_points(cv, pts)).all() and curve.unpack_points(cv, packed) == pts
    assert curve.on_curve(cv, pts[2]) and not curve.on_curve(cv, (1, 1))


@pytest.mark.parametrize("cv", CURVES)
def test_naive_msm_equals_the_known_multiple_formula(cv):
    rng = random.Random(7 + cv)
    r = mr.ORDER[cv]
    for n in (1, 2, 3, 17, 64):
        bs, pts = mr.known_bases(2 * cv, n)
        assert all(mr.on_curve(cv, p) for p in pts)
        sc = [rng.randrange(r) for _ in range(n)]
        sc[0] = r - 1
        if n > 2:
            sc[1], sc[2] = 0, 1
        assert mr.naive_msm(cv, sc, pts) == mr.expected_msm(2 * cv, sc, bs), n
        assert mr.bitwise_msm(cv, sc, pts) == mr.expected_msm(2 * cv, sc, bs), n
    bs, pts = mr.known_bases(2 * cv, 40, incremental=True)
    sc = [rng.randrange(r) for _ in range(40)]
    assert mr.naive_msm(cv, sc, pts) == mr.expected_msm(2 * cv, sc, bs)
    assert pts[5] == mr.gen_mul(cv, bs[5])


def _base_fields():
    g = _gen()
    return g, ((g.VESTA_BASE_P, g.VESTA_BASE_NP), (g.BN254_BASE_P, g.BN254_BASE_NP))


@pytest.mark.parametrize("cv", CURVES)
def test_generated_base_field_product_matches_integers(cv):
    g, fields = _base_fields()
    pw, np_ = fields[cv]
    q = _val(pw)
    assert q == mr.Q[cv] and np_ == (-pow(q, -1, 1 << 32)) % (1 << 32)
    assert pw[7] < 0x7ffffffe  # the < 2p, one-subtraction property
    rinv = pow(1 << 256, -1, q)
    rng = random.Random(50 + cv)
    crafted = fc.crafted_pairs(q)
    carry = fc.carry_pairs(q)
    print("curve %d: crafted %d / %d, carry %d / %d" % (cv, len(crafted), fc.CRAFT_TARGETS, len(carry),
                                                       fc.CARRY_TARGETS))
    assert len(crafted) >= fc.CRAFT_MIN_FOUND, (len(crafted), fc.CRAFT_TARGETS)
    assert len(carry) >= fc.CARRY_MIN_FOUND, (len(carry), fc.CARRY_TARGETS)
    cases = _edge_pairs(q) + [(c[3], c[4]) for c in crafted] + [(c[4], c[3]) for c in crafted]
    cases += [(c[1], c[2]) for c in carry]
    cases += [(rng.randrange(q), rng.randrange(q)) for _ in range(300)]
    for a, b in cases:
        assert _mont(g, pw, np_, a, b) == a * b * rinv % q, (hex(a), hex(b))


def _edge_pairs(q):
    return fc.edge_pairs(q)


def test_base_field_structs_hold_computed_constants():
    """VestaBase / Bn254Base of csrc/b2f_field.h: every constant recomputed from the modulus."""
    src = open(os.path.join(ROOT, "zk-odst_amd", "csrc", "b2f_field.h")).read()
    for name, q in (("VestaBase", mr.Q[0]), ("Bn254Base", mr.Q[1])):
        body = re.search(r"struct %s \{(.*?)\n\};" % name, src, re.S).group(1)

        def arr(field):
            m = re.search(r"uint32_t %s\[8\] = \{(.*?)\}" % field, body, re.S)
            return _val([int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")])

        R = (1 << 256) % q
        assert arr("P") == q and arr("R") == R and arr("R2") == R * R % q and arr("R3") == R * R * R % q
        assert int(re.search(r"NP = (0x\w+?)u;", body).group(1), 16) == (-pow(q, -1, 1 << 32)) % (1 << 32)
        assert int(re.search(r"RQ = (0x\w+?)ull;", body).group(1), 16) == (R << 64) // q


LENS = (1, 2, 3, 1 << 10, 1 << 17, 1 << 20, 1 << 28)


def test_msm_plan_invariants():
    from b2f import B2FError, _lib

    for form in range(4):
        for n_cols in (1, 7, 64):
            prev = 0
            for ln in LENS:
                p = _lib.msm_plan(ln, n_cols, form)
                c, w = p["window_bits"], p["windows"]
                assert 1 <= c <= 16, p
                # the scalar's bits (both moduli are below 2^255) plus the recoding carry
                assert mr.ORDER[form >> 1] < 1 << 255 and w * c >= 255 + 1 and (w - 1) * c < 256, p
                assert 1 <= p["group"] <= n_cols, p
                assert p["scratch_bytes"] >= prev > -1, (ln, p)
                prev = p["scratch_bytes"]
            assert prev < 4 << 30  # bounded whatever the call's size
    assert _lib.msm_plan(1 << 17, 7)["scratch_bytes"] <= _lib.msm_plan(1 << 17, 64)["scratch_bytes"]
    for bad in ((0, 1, 1), ((1 << 28) + 1, 1, 1), (5, 0, 1), (5, 1, 4)):
        with pytest.raises(B2FError) as e:
            _lib.msm_plan(*bad)
        assert e.value.code == _lib.ERR_ARG, bad
    # any output pointer may be null
    assert _lib.load().b2f_msm_plan(100, 1, 1, None, None, None, None) == _lib.OK


def test_msm_plan_scratch_is_monotone_across_window_changes():
    from b2f import _lib

    prev = 0
    lens = sorted({ln for k in range(0, 21) for ln in ((1 << k), (1 << k) + 1, (2 << k) - 1)})
    for ln in lens:  # both sides of every length at which the default window width changes
        sb = _lib.msm_plan(ln, 3)["scratch_bytes"]
        assert sb >= prev, ln
        prev = sb


def test_forced_msm_plan_is_honoured_and_strictly_parsed():
    from b2f import B2FError, _lib

    assert "B2F_DIAG_MSM_PLAN" not in os.environ
    default = _lib.msm_plan(300, 5)
    assert _lib.msm_plan(300, 5, diag=True) == default
    try:
        for c in (1, 2, 5, 8, 13, 16):
            os.environ["B2F_DIAG_MSM_PLAN"] = str(c)
            p = _lib.msm_plan(300, 5, diag=True)
            assert p["window_bits"] == c and p["windows"] == -(-256 // c), p
            assert _lib.msm_plan(300, 5) == default  # the product library reads no environment
        os.environ["B2F_DIAG_MSM_PLAN"] = "7,2"
        for n_cols, g in ((5, 2), (7, 2), (1, 1)):
            p = _lib.msm_plan(1 << 12, n_cols, diag=True)
            assert p["window_bits"] == 7 and p["group"] == g, p
        for bad in ("", "0", "17", "7,", "7,0", ",2", "7, 2", " 7", "07", "7,02", "-7", "+7", "7x", "7,2,1",
                    "7;2", "7,4097", "99999", "0x7"):
            os.environ["B2F_DIAG_MSM_PLAN"] = bad
            with pytest.raises(B2FError) as e:
                _lib.msm_plan(300, 5, diag=True)
            assert e.value.code == _lib.ERR_ARG, bad
        os.environ["B2F_DIAG_MSM_PLAN"] = "16,64"  # 64 groups of 2^19 buckets exceed a pass
        with pytest.raises(B2FError):
            _lib.msm_plan(300, 64, diag=True)
    finally:
        os.environ.pop("B2F_DIAG_MSM_PLAN", None)
    assert _lib.msm_plan(300, 5, diag=True) == default


def test_libraries_export_what_they_should():
    from b2f import _lib

    prod = open(_lib.LIB_PATH, "rb").read()
    diag = open(_lib.DIAG_LIB_PATH, "rb").read()
    for name in (b"B2F_DIAG_MSM_PLAN", b"b2f_debug_curve_op"):
        assert name not in prod, name
        assert name in diag, name
    for name in (b"b2f_msm_dev", b"b2f_msm_plan"):
        assert name in prod and name in diag, name
    assert hasattr(_lib.load(diag=True), "b2f_debug_curve_op")
    assert not hasattr(_lib.load(), "b2f_debug_curve_op")
    assert "b2f_debug_curve_op" in [n for n, _, _ in _lib.DIAG_SIGNATURES]
    assert len(_lib.KERNEL_NAMES) == 10
