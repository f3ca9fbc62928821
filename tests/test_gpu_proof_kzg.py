"""A BN254 proof built from the device calls and opened with KZG (SHPLONK, BDFG20 §4), judged by
tests/kzg_ref.py.

One proof at k = 17, ext_k = 19, form 3 (BN254, Montgomery), the three-instance shape (rounds 1, 0,
12; 6,092 rows). The parameters are Engine.kzg_setup(17, tau) on the device: g[i] = [tau^i] G by
b2f_fixed_base_mul_dev, g_lagrange by the group NTT; no point table is built in Python. The steps up
to the evaluations are tests/test_gpu_proof.py's Keygen and Proof, unchanged. The opening is then a
composition of calls the library already has, over the rotation sets the multiopen forms:

  h(X)   poly_combine (the x_1 folds q_i and q_i - r_i), kate_divide over each set's points,
         poly_combine with the weights v^(ns-1-i): the f_poly of the IPA path; W = msm(h, g)
  L(X)   one poly_combine of the q_i and h with the host scalars w_i Z_{T \\ S_i}(u) and -Z_T(u); its
         constant sum_i w_i Z_{T \\ S_i}(u) r_i(u) is not subtracted: kate_divide discards the
         remainder, so the floor quotient by X - u is the same; W' = msm(kate_divide(L, [u]), g)

and kzg_ref checks F == [tau - u] W' in G1 (tau is the test's: no pairing is written). What is
claimed is that equation on the device's polynomials and commitments, not byte-level agreement with
a halo2 backend's transcript.

The IPA path of test_gpu_proof.py also runs once against this g, its verifier given g_mult =
[tau^i mod r]: a set-up that is wrong in a way KZG's own check cannot see, because the prover and
the verifier share it, is caught by the verifier's G'_0 = <s, G>.

Needs an MI355X (`-m gpu`)."""
import copy
import random

import numpy as np
import pytest

import kzg_ref as kz
import msm_ref as mr
import ntt_ref as nr
import open_ref as orf
import test_gpu_proof as tgp
import verifier_ref as vr

from test_gpu_proof import COLUMNS, K, N, SMALL, USABLE, _ints, _points
from test_gpu_quotient import _dev, _random_rows, _stream, _zeta

pytestmark = pytest.mark.gpu

FORM = 3
TAU = 0x2a1f0e3d4c5b6a79880796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1


class KzgParams(tgp.Params):
    """test_gpu_proof.Params with g and g_lagrange from the device's set-up; the rest is restated
    (Params builds its g inside its constructor). g_mult, the multiples the IPA's verifier needs,
    are the powers of tau."""

    def __init__(self, engine, form, tau):
        import torch

        self.engine, self.form, self.cv = engine, form, mr.curve_of_form(form)
        self.p = nr.modulus(form)
        self.zeta = _zeta(form)
        self.tau = tau % self.p
        self.g, self.g_lagrange = engine.kzg_setup(K, self.tau, form=form)
        rng = random.Random(7100 + form)
        self.u, self.w = rng.randrange(1, self.p), rng.randrange(1, self.p)
        self.U, self.W = mr.gen_mul(self.cv, self.u), mr.gen_mul(self.cv, self.w)
        self.table = _random_rows((3, N, 4), 7110 + form)
        engine.spread_table_dev(USABLE, form, self.table.data_ptr(), N, _stream())
        self.table_c = engine.ntt_columns(self.table, K, inverse=True, form=form)
        self.table_commit = engine.msm(self.table, self.g_lagrange, form=form)
        self.l = engine.extend_columns(engine.lagrange_selectors(K, USABLE, form=form), K, tgp.EXT_K, self.zeta,
                                       form=form)
        self.table_tail = np.array(_ints(self.table[:, USABLE:], form), dtype=object).reshape(3, N - USABLE)
        assert not torch.equal(self.g, self.g_lagrange)

    @property
    def g_mult(self):
        if not hasattr(self, "_g_mult"):
            out, acc = [], 1
            for _ in range(N):
                out.append(acc)
                acc = acc * self.tau % self.p
            self._g_mult = out
        return self._g_mult


class KzgProof(tgp.Proof):
    """test_gpu_proof.Proof with the KZG opening as its `open` step (so rerun() ends in it); the IPA
    opening stays available as open_ipa()."""

    def __init__(self, keygen, seed):
        super().__init__(keygen, seed)
        self.ch["v"], self.ch["u"] = self.ch["x2"], self.ch["x3"]
        self.judge = kz.Verifier(self.v)

    def open_ipa(self):
        tgp.Proof.open(self)

    def open(self, drop_set=None):
        import torch

        eng, pr, form, p, ch = self.engine, self.pr, self.form, self.p, self.ch
        x1, v, u = ch["x1"], ch["v"], ch["u"]
        sets = [([self.points[r] for r in rots], rots, [COLUMNS.index(c) for c in cols])
                for rots, cols in vr.group_queries(self.queries)]
        ns, nc = len(sets), len(COLUMNS)
        # step 1, as the IPA path's f_poly: q_i, q_i - r_i, the division by Z_{S_i}, the fold across sets
        r_block = torch.zeros((ns, N, 4), dtype=torch.int64, device="cuda:0")
        for i, (pts, rots, members) in enumerate(sets):
            folded = [0] * len(pts)
            for m in members:
                folded = [(e * x1 + self.evals[(COLUMNS[m], r)]) % p for e, r in zip(folded, rots)]
            r_block[i, :len(pts)] = _dev(nr.pack(orf.interpolate(pts, folded, p), form))
        both = torch.cat([self.block, r_block])
        fold = [[(m, pow(x1, len(members) - 1 - i, p)) for i, m in enumerate(members)] for _, _, members in sets]
        diff = [terms + [(nc + i, p - 1)] for i, terms in enumerate(fold)]
        qd = eng.poly_combine(both, fold + diff, form=form)
        q_polys = qd[:ns].contiguous()
        quo = eng.kate_divide(qd[ns:].contiguous(), [pts for pts, _, _ in sets], form=form)
        weights = [pow(v, ns - 1 - i, p) for i in range(ns)]
        h_poly = eng.poly_combine(quo, [list(enumerate(weights))], form=form)
        # step 2: a few host field elements, one poly_combine, one division by X - u
        union = []
        for pts, _, _ in sets:
            union += [t for t in pts if t not in union]

        def vanish(pts):
            acc = 1
            for t in pts:
                acc = acc * (u - t) % p
            return acc

        terms = [(i, weights[i] * vanish([t for t in union if t not in pts]) % p)
                 for i, (pts, _, _) in enumerate(sets) if i != drop_set]
        l_poly = eng.poly_combine(torch.cat([q_polys, h_poly]), [terms + [(ns, (-vanish(union)) % p)]], form=form)
        w_quot = eng.kate_divide(l_poly, [[u]], form=form)
        opening = eng.msm(torch.cat([h_poly, w_quot]), pr.g, form=form)
        eng.sync(_stream())
        w, w_prime = _points(opening, form)
        self.n_sets = ns
        self.kzg = dict(commitments=self.commitments, evals=self.evals, ch=ch, w=w, w_prime=w_prime)

    def kzg_verdict(self):
        return self.judge.verify(self.kzg, self.pr.tau)


class Case:
    def __init__(self, engine):
        self.params = KzgParams(engine, FORM, TAU)
        self.keygen = tgp.Keygen(self.params, SMALL)
        self.proof = None

    def honest(self):
        if self.proof is None:
            self.proof = KzgProof(self.keygen, 7200 + FORM)
            self.proof.rerun("advice")
        return self.proof


@pytest.fixture(scope="module")
def case(engine):
    return Case(engine)


def test_the_parameters_are_the_powers_of_tau(case):
    """A sample of g against the big integers (all of g at k = 10: tests/test_gpu_fixed_base.py)."""
    pr = case.params
    idx = [0, 1, 2, 255, 256, 65535, 65536, N - 2, N - 1]
    got = mr.unpack_points(pr.cv, tgp._host(pr.g)[idx])
    assert got == [mr.gen_mul(pr.cv, pow(pr.tau, i, pr.p)) for i in idx]


def test_the_verifier_accepts_the_kzg_opened_proof(case):
    pf = case.honest()
    lhs, rhs = pf.identity_sides()
    assert lhs == rhs and lhs != 0
    assert pf.n_sets > 3 and pf.kzg["w"] is not None and pf.kzg["w_prime"] is not None
    assert pf.kzg_verdict() == "accept"


def test_an_altered_evaluation_is_rejected_by_the_final_check(case):
    pf = case.honest()
    proof = dict(pf.kzg, evals=dict(pf.kzg["evals"]))
    key = (("advice", 3), 0)
    proof["evals"][key] = (proof["evals"][key] + 1) % pf.p
    assert not pf.judge.opening_holds(proof, pf.pr.tau)  # the final check alone
    assert pf.judge.verify(proof, pf.pr.tau) == "identity"  # and the identity in front of it


def test_an_l_with_one_q_left_out_is_rejected(case):
    honest = case.honest()
    pf = copy.copy(honest)
    pf.open(drop_set=1)
    assert pf.kzg["w"] == honest.kzg["w"] and pf.kzg["w_prime"] != honest.kzg["w_prime"]
    assert pf.kzg_verdict() == "kzg"
    assert honest.kzg_verdict() == "accept"  # the copy left the honest proof alone


def test_a_blinding_row_that_differs_from_the_committed_cells_is_rejected(case):
    """The advice is committed from the cells with its tail; the polynomial that is evaluated and
    opened has one other blinding row. Blinding rows are free, so the identity holds; Q_i folds a
    commitment that is not the commitment of the polynomial inside q_i."""
    import b2f

    honest = case.honest()
    pf = copy.copy(honest)
    pf.adv = honest.adv.clone()
    col = b2f.halo2_column_index(9)
    pf.adv[col, USABLE + 2, 0] ^= 1
    pf.rerun("quotient")
    assert pf.commitments[("advice", col)] == honest.commitments[("advice", col)]
    assert pf.evals != honest.evals
    lhs, rhs = pf.identity_sides()
    assert lhs == rhs and lhs != 0
    assert pf.kzg_verdict() == "kzg"


def test_the_ipa_path_accepts_against_the_same_g(case):
    """The verifier computes G'_0 = <s, G> from g_mult = [tau^i mod r] on its own, so a g that is not
    the powers of tau fails here whatever the KZG check shares with the prover."""
    pf = copy.copy(case.honest())
    pf.open_ipa()
    assert pf.verdict() == "accept"
    wrong = [1] + [m + 1 for m in pf.pr.g_mult[1:]]
    assert pf.v.verify(pf.proof, dict(g=wrong, u=pf.pr.u, w=pf.pr.w)) == "ipa"
