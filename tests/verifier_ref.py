"""A verifier for proofs assembled from the prover calls of include/b2f.h, written from halo2's
verifier side (halo2_proofs 0.3.0 plonk/verifier.rs, plonk/permutation/verifier.rs,
plonk/lookup/verifier.rs, poly/multiopen/verifier.rs, poly/commitment/verifier.rs) on Python
integers and tests/msm_ref.py points. It takes commitments, evaluations and challenges; it never
sees a column. It shares no term code with tests/quotient_ref.py and carries its own field
constants; the only things it takes from elsewhere are the gate polynomials of
tests/quotient_gates_ref.py (pinned to the oracle's independent gate code) for the chip's shape.

Three checks, in halo2's order:

  identity   the vanishing identity at x: the y-fold of the gate terms, the permutation terms and
             the lookup terms, formed from the evaluations alone with closed-form l_0, l_last,
             l_active, equals (x^n - 1) sum_i x^(n i) h_i(x);
  multiopen  from the commitments and the same evaluations: per point set the x_1 fold Q_set of the
             commitments and r_set of the evaluations, the expected f(x_3), then the x_4 fold to one
             final commitment and one final value (no verdict of its own: it feeds the IPA);
  ipa        Q + sum_j (u_j^-1 L_j + u_j R_j) = [c] G'_0 + [c b_0 z] U + [f] W with Q = final
             commitment + [z v] U, b_0 = prod_j (1 + u_j x_3^(2^(k-1-j))), G'_0 = <s, G>.

What is left to the caller of the library is left out here as well: there is no transcript (the
challenges are arguments), the commitment blinds are zero and there is no s_poly masking; the
per-round l_rand / r_rand of the IPA are in, through the prover's running f.

Columns are named by pairs: ("advice", halo2 index), ("fixed", g), ("table", c), ("sigma", j),
("perm_z", s), ("lookup", 2 | 3 | 4) for A', S', z (the indices of b2f_lookup_columns_dev) and
("h", i). A query is (column, rotation), the rotation in circuit rows (negative, and usable_rows
for the permutation's link, included); its point is x omega^rotation."""
import msm_ref as mr
import quotient_gates_ref as gr

MODULUS = (mr.ORDER[0], mr.ORDER[1])  # pasta Fp, BN254 Fr: the scalar fields of Vesta and G1
GENERATOR = (5, 7)                    # multiplicative generators
TWO_ADICITY = (32, 28)
N_PERM = 8


def field_of_form(form):
    return (int(form) >> 1) & 1


def omega(f, k):
    """ROOT_OF_UNITY = g^t (p - 1 = t 2^S) squared S - k times."""
    p, s = MODULUS[f], TWO_ADICITY[f]
    return pow(pow(GENERATOR[f], (p - 1) >> s, p), 1 << (s - k), p)


def delta(f):
    return pow(GENERATOR[f], 1 << TWO_ADICITY[f], MODULUS[f])


class Shape:
    """What keygen fixes about a circuit, as far as the verifier needs it. gate_terms(adv, fix)
    returns the gate terms in order, adv(column, rotation) and fix(column) giving values."""

    def __init__(self, n_advice, n_fixed, perm_columns, lookup_inputs, gate_terms):
        assert len(perm_columns) == N_PERM and len(lookup_inputs) == 3
        self.n_advice, self.n_fixed = n_advice, n_fixed
        self.perm_columns, self.lookup_inputs = tuple(perm_columns), tuple(lookup_inputs)
        self.gate_terms = gate_terms
        seen = set()

        def record(c, r):
            seen.add((c, r))
            return 0

        self.n_gate_terms = len(gate_terms(record, lambda c: 0))
        self.gate_queries = sorted(seen)


def _chip_gate_terms(adv, fix):
    """The 74 terms q_g(x) poly in the header's order: ascending selector bit, a_i = advice column
    HALO2[i], bit 14 reading k_0 = fixed column 16."""
    def a(i, rot):
        return adv(gr.HALO2[i], rot)

    out = []
    for g in range(16):
        polys = [a(1, 0) - fix(16)] if g == 14 else gr.GATES[g](a)
        out += [fix(g) * poly for poly in polys]
    return out


def chip_shape():
    """The BLAKE2f chip: equality columns a_1..a_8, lookup inputs (a_0, a_1, a_2) = (tag, dense,
    spread), seventeen fixed columns."""
    return Shape(10, 17, [gr.HALO2[j + 1] for j in range(N_PERM)], [gr.HALO2[i] for i in range(3)],
                 _chip_gate_terms)


def group_queries(queries):
    """halo2's multiopen grouping: columns with the identical rotation set share a point set.
    Returns [(rotations, columns)], the rotations of a column and the sets in order of first
    appearance. This order is part of the proof's format: the prover folds in it too."""
    rots = {}
    for col, rot in queries:
        rots.setdefault(col, [])
        if rot not in rots[col]:
            rots[col].append(rot)
    sets = {}
    for col, rs in rots.items():
        key = tuple(sorted(rs))
        sets.setdefault(key, (tuple(rs), []))[1].append(col)
    return list(sets.values())


class Verifier:
    def __init__(self, form, k, usable_rows, chunk_len, shape):
        self.form, self.k, self.n = form, k, 1 << k
        self.f = field_of_form(form)
        self.cv = mr.curve_of_form(form)
        self.p = MODULUS[self.f]
        assert 0 < usable_rows < self.n and 1 <= chunk_len <= N_PERM
        self.usable, self.chunk_len, self.shape = usable_rows, chunk_len, shape
        self.sets = -(-N_PERM // chunk_len)
        self.omega, self.delta = omega(self.f, k), delta(self.f)

    # ---- points and queries -----------------------------------------------------------------
    def _inv(self, v):
        assert v % self.p, "division by zero: a challenge collides with the domain or a point"
        return pow(v, self.p - 2, self.p)

    def point(self, x, rot):
        return x * pow(self.omega, rot % self.n, self.p) % self.p

    def queries(self, n_h=4):
        """Every (column, rotation) the identity reads, in the order the multiopen folds them."""
        sh = self.shape
        adv = set(sh.gate_queries) | {(c, 0) for c in sh.perm_columns} | {(c, 0) for c in sh.lookup_inputs}
        q = [(("advice", c), r) for c, r in sorted(adv)]
        q += [(("fixed", g), 0) for g in range(sh.n_fixed)]
        q += [(("table", c), 0) for c in range(3)]
        q += [(("sigma", j), 0) for j in range(N_PERM)]
        for s in range(self.sets):
            q += [(("perm_z", s), 0), (("perm_z", s), 1)]
            if s < self.sets - 1:
                q.append((("perm_z", s), self.usable))
        q += [(("lookup", 2), 0), (("lookup", 2), -1), (("lookup", 3), 0), (("lookup", 4), 0), (("lookup", 4), 1)]
        q += [(("h", i), 0) for i in range(n_h)]
        return q

    # ---- the vanishing identity -------------------------------------------------------------
    def lagrange(self, x, i):
        """l_i(x) = (x^n - 1) omega^i / (n (x - omega^i))"""
        p = self.p
        wi = pow(self.omega, i, p)
        return (pow(x, self.n, p) - 1) * wi % p * self._inv(self.n * (x - wi)) % p

    def selectors(self, x):
        """(l_0, l_last, l_active) at x"""
        l_last = self.lagrange(x, self.usable)
        l_blind = sum(self.lagrange(x, i) for i in range(self.usable + 1, self.n)) % self.p
        return self.lagrange(x, 0), l_last, (1 - l_last - l_blind) % self.p

    def terms(self, evals, theta, beta, gamma, x):
        """The terms of the numerator at x in halo2's order: gates, permutation, lookup."""
        p, sh, sets = self.p, self.shape, self.sets
        l_0, l_last, l_active = self.selectors(x)

        def e(col, rot=0):
            return evals[(col, rot)]

        out = [t % p for t in sh.gate_terms(lambda c, r: e(("advice", c), r), lambda c: e(("fixed", c)))]
        # the permutation argument (plonk/permutation/verifier.rs Evaluated::expressions)
        last = ("perm_z", sets - 1)
        out.append(l_0 * (1 - e(("perm_z", 0))) % p)
        out.append(l_last * (e(last) * e(last) - e(last)) % p)
        for s in range(1, sets):
            out.append(l_0 * (e(("perm_z", s)) - e(("perm_z", s - 1), self.usable)) % p)
        coset = x  # delta^j x, j running on across the sets
        for s in range(sets):
            with_sigma, with_id = e(("perm_z", s), 1), e(("perm_z", s))
            for j in range(s * self.chunk_len, min((s + 1) * self.chunk_len, N_PERM)):
                v = e(("advice", sh.perm_columns[j]))
                with_sigma = with_sigma * (v + beta * e(("sigma", j)) + gamma) % p
                with_id = with_id * (v + beta * coset + gamma) % p
                coset = coset * self.delta % p
            out.append(l_active * (with_sigma - with_id) % p)
        # the lookup argument (plonk/lookup/verifier.rs): the compressed expressions are the
        # verifier's own, from the advice and table evaluations
        a_in = s_in = 0
        for c, t in zip(sh.lookup_inputs, range(3)):
            a_in = (a_in * theta + e(("advice", c))) % p
            s_in = (s_in * theta + e(("table", t))) % p
        ap, sp, z = e(("lookup", 2)), e(("lookup", 3)), e(("lookup", 4))
        out.append(l_0 * (1 - z) % p)
        out.append(l_last * (z * z - z) % p)
        out.append(l_active * (e(("lookup", 4), 1) * (ap + beta) * (sp + gamma) - z * (a_in + beta) * (s_in + gamma)) % p)
        out.append(l_0 * (ap - sp) % p)
        out.append(l_active * (ap - sp) * (ap - e(("lookup", 2), -1)) % p)
        assert len(out) == sh.n_gate_terms + 2 * sets + 1 + 5
        return out

    def identity_sides(self, evals, theta, beta, gamma, y, x, n_h=4):
        """(the y-fold of the terms, (x^n - 1) sum_i x^(n i) h_i(x))"""
        p = self.p
        acc = 0
        for t in self.terms(evals, theta, beta, gamma, x):
            acc = (acc * y + t) % p
        xn = pow(x, self.n, p)
        h = 0
        for i in reversed(range(n_h)):
            h = (h * xn + evals[(("h", i), 0)]) % p
        return acc, (xn - 1) * h % p

    # ---- the multiopen fold -----------------------------------------------------------------
    def multiopen(self, commitments, evals, queries, x, x1, x2, x3, x4, c_f, q_at_x3):
        """(final commitment, final value): poly/multiopen/verifier.rs"""
        p, cv = self.p, self.cv
        sets = group_queries(queries)
        assert len(q_at_x3) == len(sets)
        f_at_x3 = 0
        q_commitments = []
        for (rots, cols), q_x3 in zip(sets, q_at_x3):
            pts = [self.point(x, r) for r in rots]
            assert len(set(pts)) == len(pts)
            q_c, folded = None, [0] * len(rots)
            for col in cols:
                q_c = mr.add(cv, mr.mul(cv, x1, q_c), commitments[col])
                folded = [(v * x1 + evals[(col, r)]) % p for v, r in zip(folded, rots)]
            q_commitments.append(q_c)
            # r_set(x3) by Lagrange's formula over the set's points, and the product of (x3 - pt)
            r_x3, vanish = 0, 1
            for i, (pi, vi) in enumerate(zip(pts, folded)):
                num = den = 1
                for j, pj in enumerate(pts):
                    if j != i:
                        num, den = num * (x3 - pj) % p, den * (pi - pj) % p
                r_x3 = (r_x3 + vi * num % p * self._inv(den)) % p
                vanish = vanish * (x3 - pi) % p
            f_at_x3 = (f_at_x3 * x2 + (q_x3 - r_x3) * self._inv(vanish)) % p
        final_c, final_v = c_f, f_at_x3
        for q_c, q_x3 in zip(q_commitments, q_at_x3):
            final_c = mr.add(cv, mr.mul(cv, x4, final_c), q_c)
            final_v = (final_v * x4 + q_x3) % p
        return final_c, final_v

    # ---- the inner product argument ---------------------------------------------------------
    def ipa(self, commitment, value, x3, z, us, ls, rs, c, f, g_multiples, u_multiple, w_multiple):
        """The final identity. The generators, U and W are g_i Gen, u Gen, w Gen: the right-hand side
        is one multiple of Gen."""
        p, cv = self.p, self.cv
        assert len(us) == len(ls) == len(rs) == self.k and len(g_multiples) == self.n
        left = mr.add(cv, commitment, mr.gen_mul(cv, z * value % p * u_multiple % p))
        b_0 = 1
        for j, (u, l_pt, r_pt) in enumerate(zip(us, ls, rs)):
            left = mr.add(cv, left, mr.add(cv, mr.mul(cv, self._inv(u), l_pt), mr.mul(cv, u, r_pt)))
            b_0 = b_0 * (1 + u * pow(x3, 1 << (self.k - 1 - j), p)) % p
        s = [1]  # s_i = prod_j u_j^(bit k-1-j of i): the last round's challenge sits on bit 0
        for u in reversed(us):
            s += [v * u % p for v in s]
        g_0 = sum(si * gi for si, gi in zip(s, g_multiples)) % p
        right = (c * g_0 + c * b_0 % p * z % p * u_multiple + f * w_multiple) % p
        return left == mr.gen_mul(cv, right)

    # ---- a whole proof ----------------------------------------------------------------------
    def verify(self, proof, params):
        """"accept", or the check that rejected: "identity" or "ipa". proof: dict(commitments,
        evals, ch = dict(theta, beta, gamma, y, x, x1, x2, x3, x4, z, us), c_f, q_at_x3, ls, rs, c,
        f); params: dict(g, u, w), multiples of the generator."""
        ch = proof["ch"]
        n_h = sum(1 for col in proof["commitments"] if col[0] == "h")
        lhs, rhs = self.identity_sides(proof["evals"], ch["theta"], ch["beta"], ch["gamma"], ch["y"], ch["x"], n_h)
        if lhs != rhs:
            return "identity"
        final_c, final_v = self.multiopen(proof["commitments"], proof["evals"], self.queries(n_h), ch["x"],
                                          ch["x1"], ch["x2"], ch["x3"], ch["x4"], proof["c_f"], proof["q_at_x3"])
        if not self.ipa(final_c, final_v, ch["x3"], ch["z"], ch["us"], proof["ls"], proof["rs"], proof["c"],
                        proof["f"], params["g"], params["u"], params["w"]):
            return "ipa"
        return "accept"
