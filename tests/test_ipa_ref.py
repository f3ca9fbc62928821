"""CPU checks around the IPA opening rounds (b2f_ipa_*_dev): the restatement of tests/ipa_ref.py
against the argument's own identity, by point arithmetic that knows nothing about the points; the
header's three entry points and the ctypes table; the switch-over constant.

The identity: with Q = <p, G> + [z <p, b>] U + [f] W, every round gives
Q_next = Q + [u^-1] L_full + [u] R_full, and after the last one
Q = [c] G'_0 + [c b_0 z] U + [f] W with b_0 = prod_j (1 + u_j x^(2^(k-1-j)))."""
import random
import re

import pytest

import ipa_ref as ir
import msm_ref as mr
from conftest import ROOT


def _setup(cv, k, seed):
    r = mr.ORDER[cv]
    rng = random.Random(seed)
    n = 1 << k
    p = [rng.randrange(r) for _ in range(n)]
    x, z, f = rng.randrange(1, r), rng.randrange(1, r), rng.randrange(r)
    # generators, U and W: random multiples of the generator, used below as plain points only
    pts = [mr.mul(cv, rng.randrange(1, r), mr.GEN[cv]) for _ in range(n + 2)]
    us = [rng.randrange(1, r) for _ in range(k)]
    return p, x, z, f, pts[:n], pts[n], pts[n + 1], us


def _run(cv, k, seed, swap_l_at=None):
    """The whole loop on points. Returns (every round's invariant held, the final identity held)."""
    r = mr.ORDER[cv]
    p, x, z, f, G, U, W, us = _setup(cv, k, seed)
    b = ir.powers(cv, x, len(p))
    caller = ir.Caller(cv, U, W, z, f, seed + 1)
    q = ir.statement(cv, p, b, G, z, U, caller.f, W)
    rounds_ok = True
    for j, u in enumerate(us):
        L, R = ir.round_points(cv, p, G)
        vl, vr = ir.values(cv, p, b)
        Lf, Rf = caller.blind(L, R, vl, vr)
        if swap_l_at == j:
            Lf = mr.add(cv, Lf, mr.GEN[cv])  # another point in L_j's place
        p, b = ir.fold_scalars(cv, p, b, u)
        G = ir.fold_points(cv, G, u)
        caller.absorb(u)
        q_next = mr.add(cv, mr.add(cv, q, mr.mul(cv, pow(u, -1, r), Lf)), mr.mul(cv, u, Rf))
        rounds_ok = rounds_ok and q_next == ir.statement(cv, p, b, G, z, U, caller.f, W)
        q = q_next
    c = p[0]
    b0 = 1
    for j, u in enumerate(us):
        b0 = b0 * (1 + u * pow(x, 1 << (k - 1 - j), r)) % r
    assert len(p) == len(b) == len(G) == 1
    final = mr.add(cv, mr.add(cv, mr.mul(cv, c, G[0]), mr.mul(cv, c * b0 % r * z % r, U)), mr.mul(cv, caller.f, W))
    return rounds_ok, q == final, b[0] == b0


@pytest.mark.parametrize("cv", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_round_invariant_and_final_identity(cv, k):
    assert _run(cv, k, 40 + 10 * k + cv) == (True, True, True)


@pytest.mark.parametrize("cv", [0, 1])
def test_a_replaced_l_breaks_the_identity(cv):
    for k, at in ((1, 0), (4, 0), (4, 2), (4, 3)):
        rounds_ok, final_ok, _ = _run(cv, k, 90 + k + cv, swap_l_at=at)
        assert not rounds_ok and not final_ok, (k, at)


@pytest.mark.parametrize("cv", [0, 1])
def test_known_multiples_agree_with_point_arithmetic(cv):
    """The closed forms the GPU tests use (scalars mod r, one gen_mul) = the point arithmetic."""
    r = mr.ORDER[cv]
    rng = random.Random(70 + cv)
    k = 4
    gm = [rng.randrange(1, r) for _ in range(1 << k)]
    G = ir.points_of(cv, gm)
    p = [rng.randrange(r) for _ in range(1 << k)]
    us = [rng.randrange(1, r) for _ in range(k)]
    x = rng.randrange(r)
    b = ir.powers(cv, x, 1 << k)
    for rnd, u in zip(ir.opening_known(cv, p, x, gm, us), us):
        assert ir.round_points(cv, p, G) == (mr.gen_mul(cv, rnd["l"]), mr.gen_mul(cv, rnd["r"]))
        assert ir.values(cv, p, b) == (rnd["value_l"], rnd["value_r"])
        p, b = ir.fold_scalars(cv, p, b, u)
        G = ir.fold_points(cv, G, u)
        assert (p, b, G) == (rnd["p"], rnd["b"], ir.points_of(cv, rnd["gm"]))


def test_header_declares_and_binding_binds_the_entry_points():
    from b2f import _lib

    src = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/b2f.h").read(), flags=re.S)
    table = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    for name, n_args in (("b2f_ipa_powers_dev", 6), ("b2f_ipa_round_dev", 9), ("b2f_ipa_fold_dev", 8),
                         ("b2f_ipa_direct_max_len", 0)):
        m = re.search(r"B2F_API\s+\w+\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
        assert m, name
        args = m.group(1).strip()
        assert (0 if args == "void" else len(args.split(","))) == n_args, name
        assert name in table and len(table[name][1]) == n_args, name
        assert hasattr(_lib.load(), name) and hasattr(_lib.load(diag=True), name), name
    assert int(re.search(r"#define B2F_NUM_KERNELS\s+(\d+)", src).group(1)) == 10


def test_direct_switch_over_is_a_power_of_two_in_range():
    import os

    from b2f import _lib

    assert "B2F_DIAG_IPA_DIRECT" not in os.environ
    m = _lib.ipa_direct_max_len()
    assert 2 <= m <= 1 << 28 and m & (m - 1) == 0
    assert _lib.ipa_direct_max_len(diag=True) == m
    try:
        for v, want in (("0", 0), ("2", 2), ("4294967296", 1 << 32)):
            os.environ["B2F_DIAG_IPA_DIRECT"] = v
            assert _lib.ipa_direct_max_len(diag=True) == want
            assert _lib.ipa_direct_max_len() == m  # the product library reads no environment
    finally:
        os.environ.pop("B2F_DIAG_IPA_DIRECT", None)
    prod = open(_lib.LIB_PATH, "rb").read()
    diag = open(_lib.DIAG_LIB_PATH, "rb").read()
    assert b"B2F_DIAG_IPA_DIRECT" not in prod and b"B2F_DIAG_IPA_DIRECT" in diag
