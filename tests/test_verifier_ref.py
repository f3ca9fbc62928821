"""tests/verifier_ref.py pinned on the CPU, before any GPU is involved: a pure-Python prover at a toy
size (k = 4, ext_k = 6, five blinding rows) builds whole proofs, the verifier accepts them on both
fields and rejects each single tamper, by the check that has to see it.

The toy circuit follows the constructions of tests/test_quotient_ref.py (copy cycles over eight
equality columns, a six-row table padded with its row 0), with what the chip has and those toys
leave out: two gates whose rotations wrap around the domain (one forwards from the last usable
row to row 0, one backwards from row 0 into the blinding rows), and lookup inputs that are the
theta-compression of three advice columns into a three-column table, so the verifier has to derive
A(x) and S(x) itself. The prover interpolates with ntt_ref, forms the quotient with quotient_ref
(extend, terms, fold, divide), evaluates with open_ref.eval, commits with msm_ref on known
multiples and runs open_ref.multiopen_field_side and the ipa_ref loop. Every blinding row is
random; those of A and S are the compression of the advice and table rows there."""
import copy
import random

import numpy as np
import pytest

import ipa_ref as ir
import msm_ref as mr
import ntt_ref as nr
import open_ref as orf
import quotient_ref as qr
import verifier_ref as vr

K, EXT_K = 4, 6
N, N_EXT, ROT = 1 << K, 1 << EXT_K, 1 << (EXT_K - K)
USABLE = N - 6
CHUNK = 2
FORMS = [1, 3]

# advice columns: 0, 9, 10 the lookup's inputs; 1..8 the equality columns; 11, 12 the gates' columns
PERM_COLUMNS = (1, 2, 3, 4, 5, 6, 7, 8)
LOOKUP_INPUTS = (0, 9, 10)
WRAP = N - USABLE + 1           # from the last usable row to row 0
GATE_A_ROWS = (1, 2, 5, USABLE - 1)
GATE_B_ROWS = (0, 4)


def toy_gate_terms(adv, fix):
    """q_0 (c_11 c_11@WRAP - c_12), q_1 (c_12@3 - c_11 - c_11@-1)."""
    return [fix(0) * (adv(11, 0) * adv(11, WRAP) - adv(12, 0)),
            fix(1) * (adv(12, 3) - adv(11, 0) - adv(11, -1))]


SHAPE = vr.Shape(13, 2, PERM_COLUMNS, LOOKUP_INPUTS, toy_gate_terms)


def test_the_field_constants_are_the_package_s():
    from b2f import field

    for form in FORMS:
        f = field.of_form(form)
        assert vr.field_of_form(form) == f and vr.MODULUS[f] == field.MODULUS[f] == nr.modulus(form)
        assert vr.delta(f) == field.delta(f)
        for k in (1, 4, 17, 19):
            assert vr.omega(f, k) == field.omega(f, k)
        w = vr.omega(f, K)
        assert pow(w, N, vr.MODULUS[f]) == 1 and pow(w, N // 2, vr.MODULUS[f]) == vr.MODULUS[f] - 1


def test_the_chip_shape_reads_the_header_s_queries():
    import b2f

    sh = vr.chip_shape()
    assert sh.n_gate_terms == 74
    assert sh.gate_queries == sorted(tuple(int(v) for v in row) for row in b2f.gate_queries())
    assert sh.perm_columns == tuple(b2f.halo2_column_index(j + 1) for j in range(8))
    assert sh.lookup_inputs == tuple(b2f.halo2_column_index(i) for i in range(3))


class ToyProver:
    """One toy circuit and its proof. tamper: None, or a prover-side fault: ("swap_terms", t) folds
    terms t and t + 1 in each other's place, "theta" compresses with theta + 1, "fold_u" collapses p
    with u where u^-1 belongs."""

    def __init__(self, form, seed, tamper=None):
        self.form, self.tamper = form, tamper
        self.v = vr.Verifier(form, K, USABLE, CHUNK, SHAPE)
        self.p, self.cv = self.v.p, self.v.cv
        self.omega, self.delta = self.v.omega, self.v.delta
        self.omega_ext = vr.omega(self.v.f, EXT_K)
        self.zeta = pow(vr.GENERATOR[self.v.f], (self.p - 1) // 3, self.p)
        self.rng = np.random.default_rng(seed)
        ch = dict(zip(("theta", "beta", "gamma", "y", "x", "x1", "x2", "x3", "x4", "z"), self.rand(10)))
        ch["us"] = [u or 1 for u in self.rand(K)]
        self.ch = ch
        self.g_mult, _ = mr.known_bases(form, N, incremental=True)
        self.params = dict(g=self.g_mult, u=self.rand(1)[0], w=self.rand(1)[0])
        self.columns()
        self.quotient()
        self.open()

    def rand(self, count):
        return nr.random_elements(self.rng, count, self.p)

    def inv(self, v):
        return pow(v, self.p - 2, self.p)

    # ---- the witness and the arguments' columns, Lagrange form -----------------------------------
    def columns(self):
        p, ch = self.p, self.ch
        theta = (ch["theta"] + 1) % p if self.tamper == "theta" else ch["theta"]
        beta, gamma = ch["beta"], ch["gamma"]
        adv = [self.rand(N) for _ in range(13)]
        # the gates
        q = [[int(i in GATE_A_ROWS) for i in range(N)], [int(i in GATE_B_ROWS) for i in range(N)]]
        for i in GATE_A_ROWS:
            adv[12][i] = adv[11][i] * adv[11][(i + WRAP) % N] % p
        for i in GATE_B_ROWS:
            adv[12][(i + 3) % N] = (adv[11][i] + adv[11][(i - 1) % N]) % p
        assert not {(i + 3) % N for i in GATE_B_ROWS} & set(GATE_A_ROWS)
        # the permutation: copy cycles over the eight equality columns, as test_quotient_ref.toy_permutation
        cycles = [[(0, 1), (3, 7), (7, 2)], [(2, 0), (2, 9)], [(5, 4), (1, 4), (6, 8), (0, 5)]]
        mapping = {(j, i): (j, i) for j in range(8) for i in range(N)}
        for cyc in cycles:
            for a, b in zip(cyc, cyc[1:] + cyc[:1]):
                mapping[a] = b
                adv[PERM_COLUMNS[b[0]]][b[1]] = adv[PERM_COLUMNS[cyc[0][0]]][cyc[0][1]]
        sigma = [[pow(self.delta, mapping[(j, i)][0], p) * pow(self.omega, mapping[(j, i)][1], p) % p
                  for i in range(N)] for j in range(8)]
        z, start = [], 1
        for s in range(8 // CHUNK):
            col = [start]
            for i in range(USABLE):
                num = den = 1
                for j in range(s * CHUNK, (s + 1) * CHUNK):
                    cell = adv[PERM_COLUMNS[j]][i]
                    num = num * (cell + beta * pow(self.delta, j, p) * pow(self.omega, i, p) + gamma) % p
                    den = den * (cell + beta * sigma[j][i] + gamma) % p
                col.append(col[-1] * num * self.inv(den) % p)
            start = col[USABLE]
            z.append(col + self.rand(N - USABLE - 1))
        assert z[-1][USABLE] == 1
        # the lookup: three input columns into a three-column table, as test_quotient_ref.toy_lookup
        rows = [self.rand(3) for _ in range(6)]
        table = [[rows[i if i < 6 else 0][c] for i in range(USABLE)] + self.rand(N - USABLE) for c in range(3)]
        for i, t in enumerate(self.rng.integers(0, 6, USABLE)):
            for c, col in enumerate(LOOKUP_INPUTS):
                adv[col][i] = rows[int(t)][c]
        compress = lambda cols: [(theta * theta * a + theta * b + c) % p for a, b, c in zip(*cols)]  # noqa: E731
        a_col, s_col = compress([adv[c] for c in LOOKUP_INPUTS]), compress(table)  # blinding rows included
        ap = sorted(a_col[:USABLE])
        sp, spare = [None] * USABLE, list(s_col[:USABLE])
        for i in range(USABLE):
            if i == 0 or ap[i] != ap[i - 1]:
                sp[i] = ap[i]
                spare.remove(ap[i])
        for i in range(USABLE):
            if sp[i] is None:
                sp[i] = spare.pop()
        lz = [1]
        for i in range(USABLE):
            num = (a_col[i] + beta) * (s_col[i] + gamma) % p
            den = (ap[i] + beta) * (sp[i] + gamma) % p
            lz.append(lz[-1] * num * self.inv(den) % p)
        assert lz[USABLE] == 1
        self.lookup = [a_col, s_col, ap + self.rand(N - USABLE), sp + self.rand(N - USABLE),
                       lz + self.rand(N - USABLE - 1)]
        self.adv, self.fixed, self.table, self.sigma, self.z = adv, q, table, sigma, z

    def coeff(self, col):
        return nr.inverse(list(col), K, self.omega, 1, self.p)

    def ext(self, cols):
        return [qr.extend(c, K, EXT_K, self.omega, self.omega_ext, self.zeta, self.p) for c in cols]

    # ---- the quotient ----------------------------------------------------------------------------
    def quotient(self):
        p, ch = self.p, self.ch
        adv, fixed = self.ext(self.adv), self.ext(self.fixed)
        l = self.ext(qr.selectors(K, USABLE))
        gates = [[] for _ in range(SHAPE.n_gate_terms)]
        for i in range(N_EXT):
            for out, t in zip(gates, toy_gate_terms(lambda c, r: adv[c][(i + r * ROT) % N_EXT], lambda c: fixed[c][i])):
                out.append(t % p)
        perm = qr.permutation_terms(K, EXT_K, USABLE, l, [adv[c] for c in PERM_COLUMNS], self.ext(self.sigma),
                                    self.ext(self.z), CHUNK, self.omega_ext, self.zeta, self.delta, ch["beta"],
                                    ch["gamma"], p)
        look = qr.lookup_terms(K, EXT_K, l, self.ext(self.lookup), ch["beta"], ch["gamma"], p)
        terms = gates + perm + look
        assert all(any(t) for t in terms)
        if isinstance(self.tamper, tuple) and self.tamper[0] == "swap_terms":
            t = self.tamper[1]
            terms[t], terms[t + 1] = terms[t + 1], terms[t]
        self.n_terms = len(terms)
        h = qr.divide(qr.fold(terms, ch["y"], p), K, EXT_K, self.omega_ext, self.zeta, p)
        h = nr.inverse(h, EXT_K, self.omega_ext, self.zeta, p)
        if self.tamper is None:
            assert not any(h[3 * N - 3:])
        self.h = [h[i * N:(i + 1) * N] for i in range(N_EXT // N)]

    # ---- commitments, evaluations, the multiopen fold and the IPA ---------------------------------
    def open(self):
        p, cv, ch, form = self.p, self.cv, self.ch, self.form
        polys = {}
        for name, cols in (("advice", self.adv), ("fixed", self.fixed), ("table", self.table), ("sigma", self.sigma),
                           ("perm_z", self.z), ("h", None)):
            for c, col in enumerate(cols if cols is not None else self.h):
                polys[(name, c)] = self.coeff(col) if cols is not None else col
        for j in (2, 3, 4):
            polys[("lookup", j)] = self.coeff(self.lookup[j])
        commit = lambda poly: mr.expected_msm(form, poly, self.g_mult)  # noqa: E731
        queries = self.v.queries(len(self.h))
        evals = {(col, rot): orf.eval(polys[col], self.v.point(ch["x"], rot), p) for col, rot in queries}
        order = list(polys)
        sets = [([self.v.point(ch["x"], r) for r in rots], [order.index(c) for c in cols])
                for rots, cols in vr.group_queries(queries)]
        assert sorted(c for _, cols in vr.group_queries(queries) for c in cols) == sorted(order)
        mo = orf.multiopen_field_side([polys[c] for c in order], sets, ch["x1"], ch["x2"], ch["x3"], ch["x4"], p)
        # the opening of the final polynomial at x3
        gm = list(self.g_mult)
        U, W = mr.gen_mul(cv, self.params["u"]), mr.gen_mul(cv, self.params["w"])
        caller = ir.Caller(cv, U, W, ch["z"], 0, 77)
        pv, b = list(mo["final_poly"]), ir.powers(cv, ch["x3"], N)
        ls, rs = [], []
        for u in ch["us"]:
            l, r = ir.round_known(cv, pv, gm)
            full = caller.blind(mr.gen_mul(cv, l), mr.gen_mul(cv, r), *ir.values(cv, pv, b))
            ls.append(full[0])
            rs.append(full[1])
            half = len(pv) // 2
            folded, b = ir.fold_scalars(cv, pv, b, u)
            if self.tamper == "fold_u":
                folded = [(pv[i] + pv[half + i] * u) % p for i in range(half)]
            pv, gm = folded, ir.fold_known(cv, gm, u)
            caller.absorb(u)
        self.final_value = orf.eval(mo["final_poly"], ch["x3"], p)
        self.proof = dict(commitments={c: commit(polys[c]) for c in order}, evals=evals, ch=ch,
                          c_f=commit(mo["f_poly"]), q_at_x3=mo["q_at_x3"], ls=ls, rs=rs, c=pv[0], f=caller.f)


_HONEST = {}


def honest(form):
    if form not in _HONEST:
        _HONEST[form] = ToyProver(form, 40 + form)
    return _HONEST[form]


@pytest.mark.parametrize("form", FORMS)
def test_closed_form_selectors_are_the_interpolated_columns(form):
    """The only place the verifier's selectors meet quotient_ref.selectors."""
    v = vr.Verifier(form, K, USABLE, CHUNK, SHAPE)
    for x in nr.random_elements(np.random.default_rng(5 + form), 3, v.p):
        want = [orf.eval(nr.inverse(list(col), K, v.omega, 1, v.p), x, v.p) for col in qr.selectors(K, USABLE)]
        assert list(v.selectors(x)) == want
    for usable in (1, N - 1):
        v = vr.Verifier(form, K, usable, CHUNK, SHAPE)
        want = [orf.eval(nr.inverse(list(col), K, v.omega, 1, v.p), 3, v.p) for col in qr.selectors(K, usable)]
        assert list(v.selectors(3)) == want


def test_queries_are_grouped_by_rotation_set():
    v = vr.Verifier(1, K, USABLE, CHUNK, SHAPE)
    sets = vr.group_queries(v.queries())
    by_rots = {tuple(sorted(r)): cols for r, cols in sets}
    assert len(by_rots) == len(sets)
    assert by_rots[(0, 1, USABLE)] == [("perm_z", 0), ("perm_z", 1), ("perm_z", 2)]
    assert by_rots[(0, 1)] == [("perm_z", 3), ("lookup", 4)]
    assert by_rots[(-1, 0)] == [("lookup", 2)]
    assert by_rots[(-1, 0, WRAP)] == [("advice", 11)] and by_rots[(0, 3)] == [("advice", 12)]
    assert ("lookup", 3) in by_rots[(0,)] and ("h", 3) in by_rots[(0,)] and ("advice", 0) in by_rots[(0,)]
    assert sum(len(cols) for _, cols in sets) == 13 + 2 + 3 + 8 + 4 + 3 + 4


@pytest.mark.parametrize("form", FORMS)
def test_the_verifier_accepts_an_honest_proof(form):
    pr = honest(form)
    ch = pr.ch
    lhs, rhs = pr.v.identity_sides(pr.proof["evals"], ch["theta"], ch["beta"], ch["gamma"], ch["y"], ch["x"])
    assert lhs == rhs and lhs != 0
    final_c, final_v = pr.v.multiopen(pr.proof["commitments"], pr.proof["evals"], pr.v.queries(), ch["x"], ch["x1"],
                                      ch["x2"], ch["x3"], ch["x4"], pr.proof["c_f"], pr.proof["q_at_x3"])
    assert final_v == pr.final_value  # the verifier's folds give the value the prover's final polynomial has
    assert pr.v.verify(pr.proof, pr.params) == "accept"


def _bump(d, key, p):
    d[key] = (d[key] + 1) % p


PROOF_TAMPERS = [
    ("an advice evaluation", "identity", lambda pf, p: _bump(pf["evals"], (("advice", 11), WRAP), p)),
    ("an equality column's evaluation", "identity", lambda pf, p: _bump(pf["evals"], (("advice", 4), 0), p)),
    ("z(x)", "identity", lambda pf, p: _bump(pf["evals"], (("perm_z", 1), 0), p)),
    ("z(omega x)", "identity", lambda pf, p: _bump(pf["evals"], (("perm_z", 3), 1), p)),
    ("z(omega^usable x)", "identity", lambda pf, p: _bump(pf["evals"], (("perm_z", 2), USABLE), p)),
    ("A'(omega^-1 x)", "identity", lambda pf, p: _bump(pf["evals"], (("lookup", 2), -1), p)),
    ("a sigma evaluation", "identity", lambda pf, p: _bump(pf["evals"], (("sigma", 5), 0), p)),
    ("a table evaluation", "identity", lambda pf, p: _bump(pf["evals"], (("table", 1), 0), p)),
    ("an h piece's evaluation", "identity", lambda pf, p: _bump(pf["evals"], (("h", 2), 0), p)),
    ("a commitment", "ipa",
     lambda pf, p: pf["commitments"].__setitem__(("advice", 3), pf["commitments"][("advice", 4)])),
    ("the commitment of f", "ipa", lambda pf, p: pf.__setitem__("c_f", pf["commitments"][("h", 0)])),
    ("a claimed q_set(x3)", "ipa", lambda pf, p: pf["q_at_x3"].__setitem__(1, (pf["q_at_x3"][1] + 1) % p)),
    ("an L_j", "ipa", lambda pf, p: pf["ls"].__setitem__(2, pf["rs"][2])),
    ("c", "ipa", lambda pf, p: _bump(pf, "c", p)),
    ("f", "ipa", lambda pf, p: _bump(pf, "f", p)),
]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", PROOF_TAMPERS, ids=[c[0] for c in PROOF_TAMPERS])
def test_the_verifier_rejects_a_tampered_proof(form, case):
    _, stage, tamper = case
    pr = honest(form)
    proof = copy.deepcopy(pr.proof)
    tamper(proof, pr.p)
    assert pr.v.verify(proof, pr.params) == stage


PROVER_TAMPERS = [(("swap_terms", 0), "identity"), (("swap_terms", 1), "identity"), (("swap_terms", 5), "identity"),
                  (("swap_terms", 10), "identity"), (("swap_terms", 14), "identity"), ("theta", "identity"),
                  ("fold_u", "ipa")]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tamper,stage", PROVER_TAMPERS, ids=[str(t[0]) for t in PROVER_TAMPERS])
def test_the_verifier_rejects_a_faulty_prover(form, tamper, stage):
    """The same seed as the honest prover: the circuit and the challenges are the accepted ones."""
    pr = ToyProver(form, 40 + form, tamper)
    assert pr.n_terms == 2 + 9 + 5
    assert pr.v.verify(pr.proof, pr.params) == stage


def test_the_s_vector_is_the_fold_of_the_generators():
    """<s, G> built by doubling is what ipa_ref's fold leaves in G[0]."""
    cv, k = 0, 3
    r = mr.ORDER[cv]
    rng = random.Random(3)
    gm = [rng.randrange(1, r) for _ in range(1 << k)]
    us = [rng.randrange(1, r) for _ in range(k)]
    s = [1]
    for u in reversed(us):
        s += [v * u % r for v in s]
    folded = gm
    for u in us:
        folded = ir.fold_known(cv, folded, u)
    assert folded == [sum(a * b for a, b in zip(s, gm)) % r]
