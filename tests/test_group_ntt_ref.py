"""The big-integer reference of the group NTT (tests/group_ntt_ref.py) checked against itself, and
the host-only parts of the call: the header, the ctypes table and the Rust binding of
INTEGRATION.md agree on the two signatures; b2f_group_ntt_plan (host only) counts what the call
performs and refuses what the call refuses. No GPU."""
import ctypes
import random

import pytest

import group_ntt_ref as gn
import msm_ref as mr
from test_integration_binding import header_functions, rust_externs

KS = [1, 2, 3, 4]


def _bases(cv, n, seed):
    """n known multiples b_j G; a zero multiple (the identity) and a repeated point among them from
    n = 4 on."""
    rng = random.Random(seed)
    r = mr.ORDER[cv]
    b = [rng.randrange(1, r) for _ in range(n)]
    if n >= 4:
        b[1] = 0
        b[3] = b[2]
    return b, [mr.gen_mul(cv, v) for v in b]


@pytest.mark.parametrize("cv", [0, 1])
def test_omega_generates_the_domain(cv):
    from b2f import field

    r = mr.ORDER[cv]
    for k in (1, 2, 7, 20, gn.TWO_ADICITY[cv]):
        w = gn.omega(cv, k)
        assert pow(w, 1 << (k - 1), r) == r - 1
        assert w == field.omega(cv, k)  # the package's constant, derived there on its own


@pytest.mark.parametrize("cv", [0, 1])
def test_batched_fixed_base_multiples(cv):
    r = mr.ORDER[cv]
    ms = [0, 1, 2, r - 1, 255, 256, 1 << 255, 0] + [random.Random(7).randrange(r) for _ in range(4)]
    assert gn.gen_mul_many(cv, ms) == [mr.gen_mul(cv, m) for m in ms]
    assert gn.gen_mul_many(cv, []) == [] and gn.gen_mul_many(cv, [0, 0]) == [None, None]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("cv", [0, 1])
def test_definition_equals_the_known_multiples_shortcut(cv, inverse):
    for k in KS:
        b, pts = _bases(cv, 1 << k, 10 * k + cv)
        want = gn.transform_known(cv, b, k, inverse)
        assert all(mr.on_curve(cv, p) for p in want)
        assert gn.transform_def(cv, pts, k, inverse) == want, (cv, k, inverse)


@pytest.mark.parametrize("cv", [0, 1])
def test_inverse_then_forward_is_the_identity(cv):
    for k in KS:
        b, pts = _bases(cv, 1 << k, 50 + k)
        r = mr.ORDER[cv]
        assert gn.multiples(cv, gn.multiples(cv, b, k, True), k, False) == [v % r for v in b]
    k = 3
    b, pts = _bases(cv, 1 << k, 60)
    assert gn.transform_def(cv, gn.transform_def(cv, pts, k, True), k, False) == pts
    assert gn.transform_def(cv, gn.transform_def(cv, pts, k, False), k, True) == pts


@pytest.mark.parametrize("cv", [0, 1])
def test_all_equal_inputs_collapse_onto_the_first_output(cv):
    """The structured case the device test uses: n copies of P invert to (P, 0, 0, ..)."""
    k = 3
    p = mr.gen_mul(cv, 12345)
    assert gn.transform_def(cv, [p] * (1 << k), k, True) == [p] + [None] * ((1 << k) - 1)


def test_header_binding_and_integration_doc_agree_on_the_signatures():
    from b2f import _lib

    hdr = header_functions()
    rust, links = rust_externs()
    table = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    u32, u64p = ("val", "u32"), ("ptr_mut", "u64")
    want = {
        "b2f_group_ntt_dev": [("ptr_mut", "B2fCtx"), ("ptr_const", "u64"), u32, ("ptr_const", "u64"), u32, u32,
                              u64p, ("ptr_mut", "void")],
        "b2f_group_ntt_plan": [u32, u32, u64p, u64p],
    }
    for name, args in want.items():
        assert hdr[name] == (("val", "i32"), args), name
        assert rust[name] == hdr[name] and links[name] == "b2f", name
        res, cargs = table[name]
        assert res is ctypes.c_int and len(cargs) == len(args), name
        for (kind, base), c in zip(args, cargs):
            assert c is (ctypes.c_uint32 if (kind, base) == u32 else ctypes.c_void_p), (name, kind, base)
        assert hasattr(_lib.load(), name) and hasattr(_lib.load(diag=True), name), name
    assert _lib.NTT_FORWARD == 0 and _lib.NTT_INVERSE == 1


def test_plan_counts_the_scalar_multiplications_and_refuses_what_the_call_refuses():
    from b2f import _lib

    for form in range(4):
        for k in (1, 2, 3, 7, 12, 20, 28):
            n = 1 << k
            p = _lib.group_ntt_plan(k, form)
            assert p["scalar_muls"] == n + (n // 2) * (k - 1), (k, form)
            # the n / 2 twiddles, 32 bytes each; none at k = 1
            assert p["scratch_bytes"] == (0 if k == 1 else max(256, 16 * n)), (k, form)
    assert _lib.group_ntt_plan(20)["scalar_muls"] == 11010048  # the set-up step of a k = 20 prover
    for k, form in ((0, 1), (29, 1), (5, 4), (0, 4)):
        with pytest.raises(_lib.B2FError) as e:
            _lib.group_ntt_plan(k, form)
        assert e.value.code == _lib.ERR_ARG
    lib = _lib.load()
    assert lib.b2f_group_ntt_plan(5, 1, None, None) == _lib.OK  # either output may be null
    sm = ctypes.c_uint64(0)
    assert lib.b2f_group_ntt_plan(5, 3, ctypes.byref(sm), None) == _lib.OK and sm.value == 32 + 16 * 4
    sb = ctypes.c_uint64(0)
    assert lib.b2f_group_ntt_plan(5, 0, None, ctypes.byref(sb)) == _lib.OK and sb.value == 512
    assert lib.b2f_group_ntt_plan(29, 1, ctypes.byref(sm), ctypes.byref(sb)) == _lib.ERR_ARG
    assert (sm.value, sb.value) == (32 + 16 * 4, 512)  # a refusal writes nothing
