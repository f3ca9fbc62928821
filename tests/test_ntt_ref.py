"""The NTT reference of the GPU tests (tests/ntt_ref.py) against the O(n^2) sums of the
definition in include/b2f.h, and the domain generators b2f.field hands to the call."""
import numpy as np
import pytest

import ntt_ref as nr

from b2f import field

FIELDS = [(field.PALLAS, nr.P_PALLAS), (field.BN254, nr.P_BN254)]


@pytest.mark.parametrize("f,p", FIELDS)
@pytest.mark.parametrize("k", [1, 2, 5])
def test_reference_equals_the_definition(f, p, k):
    assert field.MODULUS[f] == p
    rng = np.random.default_rng(100 * k + f)
    n = 1 << k
    w = field.omega(f, k)
    for shift in (1, nr.random_elements(rng, 1, p)[0]):
        x = nr.random_elements(rng, n, p)
        fw = nr.forward(x, k, w, shift, p)
        assert fw == nr.forward_def(x, k, w, shift, p)
        assert nr.inverse(x, k, w, shift, p) == nr.inverse_def(x, k, w, shift, p)
        assert nr.inverse(fw, k, w, shift, p) == x
        assert nr.forward(nr.inverse(x, k, w, shift, p), k, w, shift, p) == x
        for in_len in sorted({1, n // 2, n - 1}):
            short = x[:in_len]
            assert nr.forward(short, k, w, shift, p) == nr.forward_def(short, k, w, shift, p)
            # the evaluations are those of the polynomial with these coefficients
            assert nr.forward(short, k, w, shift, p)[n - 1] == nr.horner(short, shift * pow(w, n - 1, p) % p, p)


@pytest.mark.parametrize("f,p", FIELDS)
def test_omega_is_a_primitive_root(f, p):
    for k in range(1, 29):
        assert pow(field.omega(f, k), 1 << (k - 1), p) == p - 1


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_limb_packing_round_trips(form):
    p = nr.modulus(form)
    vals = [0, 1, p - 1] + nr.random_elements(np.random.default_rng(form), 5, p)
    limbs = nr.pack(vals, form)
    assert limbs.shape == (8, 4) and nr.unpack(limbs, form) == vals
    one = int.from_bytes(limbs[1].tobytes(), "little")
    assert one == (nr.R256 % p if form & 1 else 1)


def test_binding_lists_the_call():
    from b2f import _lib

    assert _lib.KERNEL_NAMES[8] == "ntt" and (_lib.NTT_FORWARD, _lib.NTT_INVERSE) == (0, 1)
    assert "b2f_ntt_columns_dev" in [s[0] for s in _lib.SIGNATURES]
