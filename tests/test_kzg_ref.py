"""tests/kzg_ref.py pinned on the CPU, before any GPU is involved: the toy circuit and pure-Python
prover of tests/test_verifier_ref.py (k = 4, BN254) with its opening replaced by the KZG / SHPLONK
opening of kzg_ref's docstring: g[i] = [tau^i] G, polynomials as integer lists, W and W' as
commitments against g. The verifier accepts the honest proof and rejects each single tamper by the
check that has to see it.

Also the host-only parts of the new calls: the header, the ctypes table and the Rust binding of
INTEGRATION.md agree on b2f_fixed_base_mul_dev and b2f_fixed_base_plan; the plan call reports a
signed table and refuses what the call refuses; tests/fixed_base_ref.py's recoding is exact. No
GPU."""
import copy
import ctypes
import random

import pytest

import fixed_base_ref as fb
import kzg_ref as kz
import msm_ref as mr
import open_ref as orf
import test_verifier_ref as tv
import verifier_ref as vr
from test_integration_binding import header_functions, rust_externs

FORM = 3
TAU = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100f1e2


class ToyKzgProver(tv.ToyProver):
    """tamper: None; ("u_in_l", d): L is built with u + d where the proof names u; ("drop_q", i):
    set i's q_i is left out of L."""

    def __init__(self, seed, tamper=None):
        self.kzg_tamper = tamper
        super().__init__(FORM, seed)

    def open(self):
        p, ch, form, n = self.p, self.ch, self.form, tv.N
        ch["v"], ch["u"] = ch["x2"], ch["x3"]
        tau = TAU % p
        self.g_mult = [pow(tau, i, p) for i in range(n)]  # g[i] = gen_mul(tau^i)
        polys = {}
        for name, cols in (("advice", self.adv), ("fixed", self.fixed), ("table", self.table), ("sigma", self.sigma),
                           ("perm_z", self.z)):
            for c, col in enumerate(cols):
                polys[(name, c)] = self.coeff(col)
        for j in (2, 3, 4):
            polys[("lookup", j)] = self.coeff(self.lookup[j])
        for c, col in enumerate(self.h):
            polys[("h", c)] = col
        commit = lambda poly: mr.expected_msm(form, poly, self.g_mult)  # noqa: E731
        queries = self.v.queries(len(self.h))
        evals = {(col, rot): orf.eval(polys[col], self.v.point(ch["x"], rot), p) for col, rot in queries}
        sets = [([self.v.point(ch["x"], r) for r in rots], cols) for rots, cols in vr.group_queries(queries)]
        ns = len(sets)
        weights = [pow(ch["v"], ns - 1 - i, p) for i in range(ns)]
        union = []
        for pts, _ in sets:
            union += [t for t in pts if t not in union]
        # step 1: h(X) = sum_i w_i (q_i - r_i) / Z_{S_i}, W = commit(h)
        q_polys, h_poly = [], [0] * n
        for (pts, cols), w in zip(sets, weights):
            q, vals = [0] * n, [0] * len(pts)
            for col in cols:
                q = [(a * ch["x1"] + b) % p for a, b in zip(q, polys[col])]
                vals = [(val * ch["x1"] + orf.eval(polys[col], t, p)) % p for val, t in zip(vals, pts)]
            r = orf.interpolate(pts, vals, p)
            diff = [(a - b) % p for a, b in zip(q, r + [0] * (n - len(r)))]
            assert all(orf.eval(diff, t, p) == 0 for t in pts)
            quot = orf.divide_chain(diff, pts, p)
            h_poly = [(a + w * b) % p for a, b in zip(h_poly, quot)]
            q_polys.append(q)
        # step 2: L(X) without its constant, W' = commit(floor(L / (X - u)))
        u_l = ch["u"]
        if self.kzg_tamper and self.kzg_tamper[0] == "u_in_l":
            u_l = (u_l + self.kzg_tamper[1]) % p

        def vanish(pts):
            acc = 1
            for t in pts:
                acc = acc * (u_l - t) % p
            return acc

        l_poly = [(-vanish(union) * a) % p for a in h_poly]
        for i, ((pts, _), w, q) in enumerate(zip(sets, weights, q_polys)):
            if self.kzg_tamper == ("drop_q", i):
                continue
            s = w * vanish([t for t in union if t not in pts]) % p
            l_poly = [(a + s * b) % p for a, b in zip(l_poly, q)]
        self.l_at_u = orf.eval(l_poly, u_l, p)
        self.proof = dict(commitments={c: commit(polys[c]) for c in polys}, evals=evals, ch=ch, w=commit(h_poly),
                          w_prime=commit(orf.kate_division(l_poly, u_l, p) + [0]))
        self.sets, self.tau = sets, tau


_HONEST = {}


def honest():
    if "pr" not in _HONEST:
        _HONEST["pr"] = ToyKzgProver(40 + FORM)
    return _HONEST["pr"]


def test_the_verifier_accepts_an_honest_proof():
    pr = honest()
    v = kz.Verifier(pr.v)
    assert pr.l_at_u != 0  # the constant the device never subtracts: the floor quotient drops it
    assert len(pr.sets) > 3 and pr.proof["w"] is not None and pr.proof["w_prime"] is not None
    assert v.opening_holds(pr.proof, pr.tau)
    assert v.verify(pr.proof, pr.tau) == "accept"
    # the right-hand side depends on tau: another tau fails
    assert not v.opening_holds(pr.proof, (pr.tau + 1) % pr.p)


def _bump(d, key, p):
    d[key] = (d[key] + 1) % p


PROOF_TAMPERS = [
    ("an evaluation at the challenge point", "identity", lambda pf, p: _bump(pf["evals"], (("advice", 4), 0), p)),
    ("an evaluation at a rotation", "identity", lambda pf, p: _bump(pf["evals"], (("perm_z", 2), tv.USABLE), p)),
    ("W", "kzg", lambda pf, p: pf.__setitem__("w", pf["commitments"][("h", 0)])),
    ("W'", "kzg", lambda pf, p: pf.__setitem__("w_prime", pf["w"])),
    ("a member of a Q_i", "kzg",
     lambda pf, p: pf["commitments"].__setitem__(("advice", 3), pf["commitments"][("advice", 4)])),
    ("a member of a one-column Q_i", "kzg",
     lambda pf, p: pf["commitments"].__setitem__(("lookup", 2), pf["commitments"][("lookup", 3)])),
]


@pytest.mark.parametrize("case", PROOF_TAMPERS, ids=[c[0] for c in PROOF_TAMPERS])
def test_the_verifier_rejects_a_tampered_proof(case):
    _, stage, tamper = case
    pr = honest()
    v = kz.Verifier(pr.v)
    proof = copy.deepcopy(pr.proof)
    tamper(proof, pr.p)
    assert v.verify(proof, pr.tau) == stage
    assert not v.opening_holds(proof, pr.tau)  # the final check sees every one of them on its own


def test_the_u_of_l_must_be_the_u_of_the_check():
    pr = honest()
    v = kz.Verifier(pr.v)
    other = ToyKzgProver(40 + FORM, ("u_in_l", 1))
    assert other.proof["commitments"] == pr.proof["commitments"] and other.proof["w"] == pr.proof["w"]
    assert other.proof["w_prime"] != pr.proof["w_prime"]
    assert v.verify(other.proof, pr.tau) == "kzg"
    # and the same from the verifier's side: the honest proof checked with another u
    assert not v.opening_holds(pr.proof, pr.tau, u=(pr.ch["u"] + 1) % pr.p)
    # the faulty prover's proof is the honest one for its own u
    assert v.opening_holds(other.proof, pr.tau, u=(pr.ch["u"] + 1) % pr.p)


def test_r_left_out_on_the_verifier_s_side_is_seen():
    pr = honest()
    assert not kz.Verifier(pr.v).opening_holds(pr.proof, pr.tau, with_r=False)


def test_a_q_left_out_of_l_is_rejected():
    pr = honest()
    v = kz.Verifier(pr.v)
    for i in (0, len(pr.sets) - 1):
        other = ToyKzgProver(40 + FORM, ("drop_q", i))
        assert other.proof["w"] == pr.proof["w"]
        assert v.verify(other.proof, pr.tau) == "kzg"


# ---- the host-only parts of the new calls -----------------------------------------------------------


def test_header_binding_and_integration_doc_agree_on_the_signatures():
    from b2f import _lib

    hdr = header_functions()
    rust, links = rust_externs()
    table = {n: (res, args) for n, res, args in _lib.SIGNATURES}
    u32, u64 = ("val", "u32"), ("val", "u64")
    want = {
        "b2f_fixed_base_mul_dev": [("ptr_mut", "B2fCtx"), ("ptr_const", "u64"), ("ptr_const", "u64"), u64, u32,
                                   ("ptr_mut", "u64"), ("ptr_mut", "void")],
        "b2f_fixed_base_plan": [u64, u32, ("ptr_mut", "u32"), ("ptr_mut", "u32"), ("ptr_mut", "u64"),
                                ("ptr_mut", "u64")],
    }
    for name, args in want.items():
        assert hdr[name] == (("val", "i32"), args), name
        assert rust[name] == hdr[name] and links[name] == "b2f", name
        res, cargs = table[name]
        assert res is ctypes.c_int and len(cargs) == len(args), name
        for (kind, base), c in zip(args, cargs):
            assert c is {u32: ctypes.c_uint32, u64: ctypes.c_uint64}.get((kind, base), ctypes.c_void_p), (name, kind, base)
        assert hasattr(_lib.load(), name) and hasattr(_lib.load(diag=True), name), name


def test_plan_reports_a_signed_table_and_refuses_what_the_call_refuses():
    from b2f import _lib

    for form in range(4):
        for ln in (1, 2, 4099, 1 << 20, 1 << 28):
            p = _lib.fixed_base_plan(ln, form)
            c, w = p["window_bits"], p["windows"]
            assert 2 <= c <= 16 and c * w >= 255, p     # the digits cover every reduced scalar
            assert p["table_points"] == w * (1 << (c - 1)), p  # signed digits: half of each window stored
            assert p["scratch_bytes"] == 64 * p["table_points"], p
    for ln, form in ((0, 1), ((1 << 28) + 1, 1), (5, 4), (0, 4), (5, 1 << 31)):
        with pytest.raises(_lib.B2FError) as e:
            _lib.fixed_base_plan(ln, form)
        assert e.value.code == _lib.ERR_ARG
    lib = _lib.load()
    assert lib.b2f_fixed_base_plan(5, 1, None, None, None, None) == _lib.OK  # any output may be null
    c, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
    tp, sb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.b2f_fixed_base_plan(5, 3, ctypes.byref(c), None, None, None) == _lib.OK and c.value
    assert lib.b2f_fixed_base_plan(5, 0, None, ctypes.byref(w), ctypes.byref(tp), None) == _lib.OK
    assert tp.value == w.value << (c.value - 1)
    assert lib.b2f_fixed_base_plan(5, 2, None, None, None, ctypes.byref(sb)) == _lib.OK and sb.value == 64 * tp.value
    before = (c.value, w.value, tp.value, sb.value)
    assert lib.b2f_fixed_base_plan(0, 1, ctypes.byref(c), ctypes.byref(w), ctypes.byref(tp),
                                   ctypes.byref(sb)) == _lib.ERR_ARG
    assert (c.value, w.value, tp.value, sb.value) == before  # a refusal writes nothing


@pytest.mark.parametrize("cv", [0, 1])
def test_the_recoding_is_exact_and_never_carries_out_for_a_reduced_scalar(cv):
    from b2f import _lib

    p = _lib.fixed_base_plan(1, 2 * cv)
    c, w = p["window_bits"], p["windows"]
    r = mr.ORDER[cv]
    half = 1 << (c - 1)
    assert r < 1 << (c * w - 1)  # the top digit's own bits stay below 2^(c-1): no carry leaves it
    rng = random.Random(11 + cv)
    edge = [0, 1, r - 1, r - 2, (r - 1) // 2, sum(half << (i * c) for i in range(w)) % r,
            sum((half + 1) << (i * c) for i in range(w)) % r, (1 << (c * w - 1)) - 1]
    for s in edge + [rng.randrange(r) for _ in range(200)]:
        d = fb.recode(s, c, w)
        assert fb.value(d, c) == s and all(-half < x <= half for x in d), hex(s)
    with pytest.raises(OverflowError):
        fb.recode((1 << (c * w)) - 1, c, w)
    dbl = fb.doubling_scalar(c, w, r)
    assert fb.meets(dbl, c, w, r) == {"double"} and fb.meets(r, c, w, r) == {"cancel"}
    assert fb.expected(2 * cv, [0, 1, r - 1], 5) == [None, mr.gen_mul(cv, 5), mr.gen_mul(cv, r - 5)]
