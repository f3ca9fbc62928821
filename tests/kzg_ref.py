"""The verifier side of a KZG / SHPLONK opening (BDFG20 §4) of a proof assembled from the prover
calls of include/b2f.h, on Python integers and tests/msm_ref.py points. It takes commitments,
evaluations, challenges, the two opening points W and W' and tau; it never sees a column.

The vanishing identity and the rotation sets are tests/verifier_ref.py's (identity_sides, queries,
group_queries); the folds and the final check are written here and share nothing with
Verifier.multiopen or the prover.

Notation, over the sets of group_queries in their order, ns of them:
  S_i      the points x omega^rot of set i; T their union
  Q_i      the x_1-fold of the set's commitments, Q = Q x_1 + C in the set's column order
  r_i      the polynomial of degree < |S_i| through the same fold of the evaluations
  w_i      the weight of set i across sets: v^(ns - 1 - i), the Horner order halo2's multiopen
           folds its sets in (f = f x_2 + ...), which the prover's h(X) follows
  Z_A(u)   prod_{t in A} (u - t)

The prover sends W = [h(tau)] G with h(X) = sum_i w_i (q_i(X) - r_i(X)) / Z_{S_i}(X), takes u, and
sends W' = [((L(X) - L(u)) / (X - u))(tau)] G with
  L(X) = sum_i w_i Z_{T \\ S_i}(u) (q_i(X) - r_i(u)) - Z_T(u) h(X),
which vanishes at u when every q_i - r_i vanishes on S_i. The verifier forms
  F = sum_i w_i Z_{T \\ S_i}(u) (Q_i - [r_i(u)] G) - [Z_T(u)] W
and accepts iff e(F + [u] W', G2) = e(W', [tau] G2). Here tau is known (the set-up is the unsafe
one, Engine.kzg_setup), so the same equation is checked in G1 alone: F == [tau - u] W'. No pairing
and no G2 arithmetic is written.

Not claimed: byte-level agreement with any halo2 backend's transcript or challenge naming. The
transcript is the caller's, as everywhere in this library; what is checked is the scheme's
equation on the device's polynomials and commitments.

proof: dict(commitments, evals, ch = dict(theta, beta, gamma, y, x, x1, v, u), w, w_prime)."""
import msm_ref as mr
import verifier_ref as vr


class Verifier:
    def __init__(self, plonk):
        """plonk: the verifier_ref.Verifier of the circuit (its field, domain and queries)."""
        self.plonk = plonk
        self.p, self.cv = plonk.p, plonk.cv

    def _inv(self, v):
        assert v % self.p, "division by zero: a challenge collides with a point"
        return pow(v, self.p - 2, self.p)

    def folds(self, commitments, evals, queries, x, x1):
        """Per set: (points, Q_i, the folded evaluations at the points)."""
        p, cv = self.p, self.cv
        out = []
        for rots, cols in vr.group_queries(queries):
            pts = [self.plonk.point(x, r) for r in rots]
            assert len(set(pts)) == len(pts)
            q_c, vals = None, [0] * len(rots)
            for col in cols:
                q_c = mr.add(cv, mr.mul(cv, x1, q_c), commitments[col])
                vals = [(val * x1 + evals[(col, r)]) % p for val, r in zip(vals, rots)]
            out.append((pts, q_c, vals))
        return out

    def interpolated_at(self, pts, vals, u):
        """r(u) for the r of degree < len(pts) with r(pts[i]) = vals[i], by Lagrange's formula."""
        p = self.p
        acc = 0
        for i, (pi, vi) in enumerate(zip(pts, vals)):
            num = den = 1
            for j, pj in enumerate(pts):
                if j != i:
                    num, den = num * (u - pj) % p, den * (pi - pj) % p
            acc = (acc + vi * num % p * self._inv(den)) % p
        return acc

    def vanish_at(self, pts, u):
        acc = 1
        for t in pts:
            acc = acc * (u - t) % self.p
        return acc

    def opening_holds(self, proof, tau, u=None, with_r=True):
        """The final check alone: F == [tau - u] W'. u: the challenge the verifier uses (default:
        the proof's); with_r=False leaves the [r_i(u)] G terms out of F, which no honest proof
        survives."""
        p, cv, ch = self.p, self.cv, proof["ch"]
        u = ch["u"] if u is None else u
        n_h = sum(1 for col in proof["commitments"] if col[0] == "h")
        sets = self.folds(proof["commitments"], proof["evals"], self.plonk.queries(n_h), ch["x"], ch["x1"])
        union = []
        for pts, _, _ in sets:
            union += [t for t in pts if t not in union]
        f_pt, const, weight = None, 0, 1
        for pts, q_c, vals in reversed(sets):  # the last set carries v^0
            z_rest = self.vanish_at([t for t in union if t not in pts], u)
            s = weight * z_rest % p
            f_pt = mr.add(cv, f_pt, mr.mul(cv, s, q_c))
            if with_r:
                const = (const + s * self.interpolated_at(pts, vals, u)) % p
            weight = weight * ch["v"] % p
        f_pt = mr.add(cv, f_pt, mr.neg(cv, mr.gen_mul(cv, const)))
        f_pt = mr.add(cv, f_pt, mr.neg(cv, mr.mul(cv, self.vanish_at(union, u), proof["w"])))
        return f_pt == mr.mul(cv, (tau - u) % p, proof["w_prime"])

    def verify(self, proof, tau):
        """"accept", or the check that rejected: "identity" or "kzg"."""
        ch = proof["ch"]
        n_h = sum(1 for col in proof["commitments"] if col[0] == "h")
        lhs, rhs = self.plonk.identity_sides(proof["evals"], ch["theta"], ch["beta"], ch["gamma"], ch["y"], ch["x"],
                                             n_h)
        if lhs != rhs:
            return "identity"
        return "accept" if self.opening_holds(proof, tau) else "kzg"
