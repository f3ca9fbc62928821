"""A whole proof built from the device calls, judged by tests/verifier_ref.py.

One proof, all on one engine and one stream, at the smallest size at which it can exist (k = 17,
ext_k = 19: the spread lookup needs 2^16 usable rows, five blinding factors leave 2^17 - 6, the
largest degree is 4):

  fill          DeviceBatch.fill
  parameters    g = 2^17 known multiples of the generator, g_lagrange = Engine.g_to_lagrange(g)
  commitments   advice straight from the cells (commit_advice: len = usable, the six blinding rows
                as the tail) and fixed (commit_fixed) against g_lagrange; the table, sigma, z, A',
                S' and the lookup z by Engine.msm of their Lagrange columns against g_lagrange; the
                rows the column calls leave unwritten hold random values, those of A and S the
                compression of the advice and table rows there
  quotient      inverse NTT, extension with ZETA, gates then permutation then lookup into one h in
                place, the vanishing divide, inverse NTT; the four pieces are the stride-n view,
                committed against g
  evaluations   Engine.poly_eval on the coefficient columns at field.rotated_points
  multiopen     poly_combine / kate_divide / poly_eval over the real point sets
  IPA           ipa_powers / ipa_round / ipa_fold on a copy of g, the rounds' randomness from
                ipa_ref.Caller

Only the commitments, the evaluations, L_j / R_j, the rounds' values and c cross to the host (and the
eighteen blinding cells the compression of A and S needs); no column is unpacked. The verifier
takes them with the challenges and accepts. Each negative control is one wrong value, rebuilt from
where it enters, and is rejected by the check named in its test. Sizes above k = 17 are not run.

Needs an MI355X (`-m gpu`)."""
import copy
import random

import numpy as np
import pytest

import ipa_ref as ir
import msm_ref as mr
import ntt_ref as nr
import open_ref as orf
import verifier_ref as vr

from conftest import random_inputs
from test_gpu_quotient import _dev, _host, _random_rows, _stream, _zeta

pytestmark = pytest.mark.gpu

K, EXT_K, CHUNK = 17, 19, 2
N = 1 << K
USABLE = N - 6
SETS = 8 // CHUNK
SMALL, FULL = "rounds 1, 0, 12", "25 instances of 12 rounds"
COLUMNS = ([("advice", c) for c in range(10)] + [("fixed", c) for c in range(17)] + [("table", c) for c in range(3)]
           + [("sigma", c) for c in range(8)] + [("perm_z", c) for c in range(SETS)]
           + [("lookup", c) for c in (2, 3, 4)] + [("h", c) for c in range(4)])


def _inputs(shape):
    if shape == FULL:
        return random_inputs(25, (12,), 63)
    x = random_inputs(3, (0,), 61)
    x["rounds"] = np.asarray([1, 0, 12], dtype=np.uint32)
    return x


def _ints(t, form):
    return nr.unpack(_host(t).reshape(-1, 4), form)


def _points(t, form):
    return mr.unpack_points(mr.curve_of_form(form), _host(t))


class Params:
    """What does not depend on the circuit: g, g_lagrange, U, W, the table columns, the selectors."""

    def __init__(self, engine, form):
        import torch

        self.engine, self.form, self.cv = engine, form, mr.curve_of_form(form)
        self.p = nr.modulus(form)
        self.zeta = _zeta(form)
        self.g_mult, pts = mr.known_bases(form, N, incremental=True)
        self.g = _dev(mr.pack_points(self.cv, pts))
        self.g_lagrange = engine.g_to_lagrange(self.g, K, form=form)
        rng = random.Random(7100 + form)
        self.u, self.w = rng.randrange(1, self.p), rng.randrange(1, self.p)
        self.U, self.W = mr.gen_mul(self.cv, self.u), mr.gen_mul(self.cv, self.w)
        self.table = _random_rows((3, N, 4), 7110 + form)  # the rows past usable stay random
        engine.spread_table_dev(USABLE, form, self.table.data_ptr(), N, _stream())
        self.table_c = engine.ntt_columns(self.table, K, inverse=True, form=form)
        self.table_commit = engine.msm(self.table, self.g_lagrange, form=form)
        self.l = engine.extend_columns(engine.lagrange_selectors(K, USABLE, form=form), K, EXT_K, self.zeta, form=form)
        self.table_tail = np.array(_ints(self.table[:, USABLE:], form), dtype=object).reshape(3, N - USABLE)
        assert not torch.equal(self.g, self.g_lagrange)


class Keygen:
    """What depends on the row map alone: the fixed columns and sigma, with their commitments. The
    batch is filled here: the fill writes the fixed column."""

    def __init__(self, params, shape):
        import b2f
        import torch

        self.params = pr = params
        eng, form = pr.engine, pr.form
        self.batch = b2f.DeviceBatch(_inputs(shape))
        self.batch.fill(eng)
        self.used = int(self.batch.offsets_host[-1])
        assert self.used == {SMALL: 6092, FULL: 130500}[shape] and self.used <= USABLE
        fixed = torch.zeros((17, N, 4), dtype=torch.int64, device="cuda:0")
        self.batch.export_fixed_fp(eng, 0, self.used, form=form, out=fixed)
        sigma = self.batch.permutation_sigma(eng, K, form=form)
        both = torch.cat([fixed, sigma])
        self.coeff = eng.ntt_columns(both, K, inverse=True, form=form)       # fixed 0..16, sigma 17..24
        ext = eng.ntt_columns(self.coeff, EXT_K, shift=pr.zeta, in_len=N, form=form)
        self.fixed_e, self.sigma_e = ext[:17].contiguous(), ext[17:].contiguous()
        self.fixed_commit = self.batch.commit_fixed(eng, 0, USABLE, pr.g_lagrange, form=form)
        self.sigma_commit = eng.msm(sigma, pr.g_lagrange, form=form)


class Proof:
    """The witness-dependent steps, each leaving what the later ones read, so that a control reruns
    a copy from the step its change enters."""

    def __init__(self, keygen, seed):
        self.kg, self.pr = keygen, keygen.params
        self.engine, self.form, self.p = self.pr.engine, self.pr.form, self.pr.p
        self.seed = seed
        rng = random.Random(seed)
        names = ("theta", "beta", "gamma", "y", "x", "x1", "x2", "x3", "x4", "z")
        self.ch = {name: rng.randrange(2, self.p) for name in names}
        self.ch["us"] = [rng.randrange(2, self.p) for _ in range(K)]
        self.v = vr.Verifier(self.form, K, USABLE, CHUNK, vr.chip_shape())

    def rerun(self, first):
        steps = ["advice", "arguments", "quotient", "evaluate", "open"]
        for name in steps[steps.index(first):]:
            getattr(self, name)()
        return self

    # ---- the advice: exported for the polynomials, committed from the cells ----------------------
    def advice(self):
        import torch

        eng, batch, form = self.engine, self.kg.batch, self.form
        adv = torch.zeros((10, N, 4), dtype=torch.int64, device="cuda:0")
        batch.export_fp(eng, 0, self.kg.used, form=form, out=adv)
        tail = _random_rows((10, N - USABLE, 4), self.seed + 1)  # the six blinding rows
        adv[:, USABLE:] = tail
        self.adv = adv
        self.adv_commit = batch.commit_advice(eng, 0, USABLE, self.pr.g_lagrange, tail=tail, form=form)

    # ---- the permutation's and the lookup's columns ----------------------------------------------
    def arguments(self):
        import torch

        eng, batch, form, p, ch = self.engine, self.kg.batch, self.form, self.p, self.ch
        _, z = batch.permutation_columns(eng, K, USABLE, ch["beta"], ch["gamma"], chunk_len=CHUNK, form=form,
                                         sigma=False)
        z[:, USABLE + 1:] = _random_rows((SETS, N - USABLE - 1, 4), self.seed + 2)
        cols = torch.zeros((5, N, 4), dtype=torch.int64, device="cuda:0")
        begin = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        bad = torch.empty(1, dtype=torch.int64, device="cuda:0")
        eng.lookup_columns_dev(batch.advice.data_ptr(), batch.total_rows, begin.data_ptr(), 1, USABLE, ch["theta"],
                               ch["beta"], ch["gamma"], form, cols.data_ptr(), N, bad.data_ptr(), _stream())
        cols[2:4, USABLE:] = _random_rows((2, N - USABLE, 4), self.seed + 3)
        cols[4, USABLE + 1:] = _random_rows((N - USABLE - 1, 4), self.seed + 4)
        # A and S past the usable rows: the compression of the advice and table rows there
        inputs = torch.tensor(list(self.v.shape.lookup_inputs), device="cuda:0")
        a_tail = np.array(_ints(self.adv[inputs][:, USABLE:], form), dtype=object).reshape(3, N - USABLE)
        th = ch["theta"]
        for j, rows in ((0, a_tail), (1, self.pr.table_tail)):
            cols[j, USABLE:] = _dev(nr.pack([(th * th * a + th * b + c) % p for a, b, c in zip(*rows)], form))
        self.z, self.lookup, self.first_bad = z, cols, bad
        self.arg_commit = eng.msm(torch.cat([z, cols[2:]]), self.pr.g_lagrange, form=form)

    # ---- the quotient ----------------------------------------------------------------------------
    def pieces_of(self, coeff):
        return coeff.reshape(4, N, 4)  # the h pieces: columns of stride n

    def quotient(self):
        import torch

        eng, kg, pr, form, ch = self.engine, self.kg, self.pr, self.form, self.ch
        self.wit_c = eng.ntt_columns(torch.cat([self.adv, self.z, self.lookup]), K, inverse=True, form=form)
        ext = eng.ntt_columns(self.wit_c, EXT_K, shift=pr.zeta, in_len=N, form=form)
        adv_e, z_e, lookup_e = ext[:10].contiguous(), ext[10:10 + SETS].contiguous(), ext[10 + SETS:].contiguous()
        h = eng.quotient_gates(K, EXT_K, adv_e, kg.fixed_e, ch["y"], form=form)
        eng.quotient_permutation(K, EXT_K, USABLE, pr.l, adv_e, kg.sigma_e, z_e, CHUNK, pr.zeta, ch["beta"],
                                 ch["gamma"], ch["y"], h=h, form=form)
        eng.quotient_lookup(K, EXT_K, pr.l, lookup_e, ch["beta"], ch["gamma"], ch["y"], h=h, form=form)
        eng.quotient_divide(K, EXT_K, pr.zeta, h, form=form)
        coeff = eng.ntt_columns(h[None], EXT_K, inverse=True, shift=pr.zeta, form=form)
        self.pieces = self.pieces_of(coeff)
        self.h_commit = eng.msm(self.pieces, pr.g, form=form)

    # ---- the evaluations -------------------------------------------------------------------------
    def evaluate(self):
        import torch
        from b2f import field

        eng, kg, pr, form = self.engine, self.kg, self.pr, self.form
        wc = self.wit_c
        # COLUMNS' order: advice, fixed, table, sigma, z, A' S' z, the pieces (A and S are not opened)
        self.block = torch.cat([wc[:10], kg.coeff[:17], pr.table_c, kg.coeff[17:], wc[10:10 + SETS],
                                wc[10 + SETS + 2:], self.pieces])
        assert self.block.shape[0] == len(COLUMNS)
        self.queries = self.v.queries()
        self.rots = sorted({r for _, r in self.queries})
        assert self.rots == [-1] + list(range(12)) + [USABLE]
        self.points = dict(zip(self.rots, field.rotated_points(field.of_form(form), self.ch["x"], K, self.rots)))
        got = eng.poly_eval(self.block, [self.points[r] for r in self.rots],
                            [(COLUMNS.index(c), self.rots.index(r)) for c, r in self.queries], form=form)
        commit = torch.cat([self.adv_commit, kg.fixed_commit, pr.table_commit, kg.sigma_commit, self.arg_commit,
                            self.h_commit])
        eng.sync(_stream())
        self.evals = dict(zip(self.queries, _ints(got, form)))
        self.commitments = dict(zip(COLUMNS, _points(commit, form)))

    def identity_sides(self):
        ch = self.ch
        return self.v.identity_sides(self.evals, ch["theta"], ch["beta"], ch["gamma"], ch["y"], ch["x"])

    # ---- the multiopen folds and the IPA ---------------------------------------------------------
    def open(self):
        import torch

        eng, pr, form, p, ch, cv = self.engine, self.pr, self.form, self.p, self.ch, self.pr.cv
        x1, x2, x3, x4 = ch["x1"], ch["x2"], ch["x3"], ch["x4"]
        sets = [([self.points[r] for r in rots], rots, [COLUMNS.index(c) for c in cols])
                for rots, cols in vr.group_queries(self.queries)]
        ns, nc = len(sets), len(COLUMNS)
        # r_set: the interpolation of the x_1-folded evaluations, a few elements, on the host
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
        f_poly = eng.poly_combine(quo, [[(i, pow(x2, ns - 1 - i, p)) for i in range(ns)]], form=form)
        q_at_x3 = eng.poly_eval(q_polys, [x3], [(i, 0) for i in range(ns)], form=form)
        final = eng.poly_combine(torch.cat([q_polys, f_poly]),
                                 [[(ns, pow(x4, ns, p))] + [(i, pow(x4, ns - 1 - i, p)) for i in range(ns)]], form=form)
        c_f = eng.msm(f_poly, pr.g, form=form)
        # the opening of the final polynomial at x_3
        pv, b, g = final[0], eng.ipa_powers(x3, N, form=form), pr.g.clone()
        caller = ir.Caller(cv, pr.U, pr.W, ch["z"], 0, self.seed + 5)
        ls, rs = [], []
        ln = N
        for u in ch["us"]:
            lr, values = eng.ipa_round(pv, b, g, len=ln, form=form)
            eng.sync(_stream())
            full = caller.blind(*_points(lr, form), *_ints(values, form))
            ls.append(full[0])
            rs.append(full[1])
            eng.ipa_fold(pv, b, g, u, len=ln, form=form)
            caller.absorb(u)
            ln //= 2
        eng.sync(_stream())
        self.proof = dict(commitments=self.commitments, evals=self.evals, ch=ch, c_f=_points(c_f, form)[0],
                          q_at_x3=_ints(q_at_x3, form), ls=ls, rs=rs, c=_ints(pv[:1], form)[0], f=caller.f)

    def verdict(self):
        return self.v.verify(self.proof, dict(g=self.pr.g_mult, u=self.pr.u, w=self.pr.w))


CASES = [(1, SMALL), (3, SMALL), (1, FULL)]


class Cases:
    """The keygen part of every case, built once for the module: per form g, g_lagrange, the table
    and the selectors, per case the fixed columns and sigma, all with their commitments. The accepted
    proof of a case is built at its first use; the controls start from copies of it."""

    def __init__(self, engine):
        params = {form: Params(engine, form) for form in sorted({form for form, _ in CASES})}
        self.keygen = {(form, shape): Keygen(params[form], shape) for form, shape in CASES}
        self.proofs = {}

    def honest(self, form, shape, opened=True):
        key = (form, shape)
        if key not in self.proofs:
            pf = self.proofs[key] = Proof(self.keygen[key], 7200 + form)
            for name in ("advice", "arguments", "quotient", "evaluate"):
                getattr(pf, name)()
        if opened and not hasattr(self.proofs[key], "proof"):
            self.proofs[key].open()
        return self.proofs[key]


@pytest.fixture(scope="module")
def cases(engine):
    return Cases(engine)


CASE_IDS = ["pasta-3-instances", "bn254-3-instances", "pasta-25-instances"]


@pytest.mark.parametrize("form,shape", CASES, ids=CASE_IDS)
def test_the_identity_holds_on_the_device_s_evaluations(cases, form, shape):
    pf = cases.honest(form, shape, opened=False)
    assert int(pf.first_bad[0]) == -1  # UINT64_MAX: every input row is a table row
    assert _ints(pf.z[SETS - 1, USABLE:USABLE + 1], form) == [1]
    lhs, rhs = pf.identity_sides()
    assert lhs == rhs and lhs != 0
    # the quotient has degree <= 3n - 4: the fourth piece is the zero polynomial, its commitment the identity
    assert [c for c in COLUMNS if pf.commitments[c] is None] == [("h", 3)]
    witness = [c for c in COLUMNS[:-1] if c[0] in ("advice", "perm_z", "lookup", "h")]
    assert len({pf.commitments[c] for c in witness}) == len(witness)


@pytest.mark.parametrize("form,shape", CASES, ids=CASE_IDS)
def test_the_verifier_accepts_the_device_s_proof(cases, form, shape):
    """The multiopen folds and the 17 IPA rounds on the device, then the whole verifier. The time is the
    host's: some 170 msm_ref.mul between ipa_ref.Caller and the verifier's folds."""
    assert cases.honest(form, shape).verdict() == "accept"


def _rejected_by_the_identity(pf):
    lhs, rhs = pf.identity_sides()
    assert lhs != rhs
    assert pf.v.verify(dict(commitments=pf.commitments, evals=pf.evals, ch=pf.ch), None) == "identity"


def _with_flipped_cell(cases, a_i, row, check):
    """The honest case with one advice cell flipped in the trace before anything is committed:
    everything that reads the cells is rebuilt."""
    honest = cases.honest(1, SMALL, opened=False)
    cells = honest.kg.batch.advice
    saved = cells[a_i, row].item()
    cells[a_i, row] = saved ^ 1
    try:
        pf = copy.copy(honest)
        for name in ("advice", "arguments", "quotient", "evaluate"):
            getattr(pf, name)()
        check(pf, honest)
    finally:
        cells[a_i, row] = saved
        honest.engine.sync(_stream())


def test_an_advice_cell_flipped_in_an_enabled_gate_row_fails_the_identity(cases):
    """Row 164 of a_9, the carry of the first ADD3 block: flipped in the cells, so the commitment is
    honest and only the identity fails."""
    import b2f

    honest = cases.honest(1, SMALL, opened=False)
    assert (int(honest.kg.batch.fixed[164].item()) >> 3) & 1
    pf = copy.copy(honest)
    cells = honest.kg.batch.advice
    saved = cells[9, 164].item()
    cells[9, 164] = saved ^ 1
    try:
        pf.advice()   # a_9 is in neither argument: z and the lookup columns stand
        pf.quotient()
        pf.evaluate()
    finally:
        cells[9, 164] = saved
    h9 = ("advice", b2f.halo2_column_index(9))
    assert pf.commitments[h9] != honest.commitments[h9]
    assert {c for c in COLUMNS if pf.commitments[c] != honest.commitments[c]} <= {h9} | {("h", i) for i in range(4)}
    _rejected_by_the_identity(pf)


def test_a_cell_of_an_equality_column_inside_a_copy_class_fails_the_identity(cases):
    import b2f

    # the first copy of the one-round instance between columns outside the lookup: a_4 <- a_7
    dst_row, dst_col, src_row, src_col = next(tuple(int(v) for v in c) for c in b2f.copy_constraints(1)
                                              if c[1] >= 3 and c[3] >= 3)
    assert (dst_row, dst_col, src_row, src_col) == (192, 4, 180, 7)

    def check(pf, honest):
        assert int(pf.first_bad[0]) == -1
        assert _ints(pf.z[SETS - 1, USABLE:USABLE + 1], 1) != [1]  # the grand product does not close
        _rejected_by_the_identity(pf)

    _with_flipped_cell(cases, dst_col, dst_row, check)


def test_a_spread_cell_that_is_no_table_row_fails_the_identity(cases):
    row = 3000

    def check(pf, honest):
        assert int(pf.first_bad[0]) == row  # halo2's ConstraintSystemFailure; the columns are meaningless
        _rejected_by_the_identity(pf)

    _with_flipped_cell(cases, 2, row, check)


def test_an_altered_z_cell_of_the_last_set_fails_the_identity(cases):
    honest = cases.honest(1, SMALL, opened=False)
    pf = copy.copy(honest)
    pf.z = honest.z.clone()
    pf.z[SETS - 1, 4000, 0] ^= 1
    import torch

    pf.arg_commit = pf.engine.msm(torch.cat([pf.z, pf.lookup[2:]]), pf.pr.g_lagrange, form=pf.form)
    pf.quotient()
    pf.evaluate()
    last = ("perm_z", SETS - 1)
    assert {c for c in COLUMNS if pf.commitments[c] != honest.commitments[c]} == {last} | {("h", i) for i in range(4)}
    _rejected_by_the_identity(pf)


def test_a_blinding_row_that_differs_from_the_committed_cells_fails_the_ipa(cases):
    """The advice is committed from the cells with its tail; the polynomial that is extended, evaluated
    and opened has one other blinding row. Blinding rows are free, so the identity holds; the final
    commitment the verifier folds is not the commitment of the polynomial the IPA opens."""
    import b2f

    honest = cases.honest(1, SMALL, opened=False)
    pf = copy.copy(honest)
    pf.adv = honest.adv.clone()
    pf.adv[b2f.halo2_column_index(9), USABLE + 2, 0] ^= 1
    pf.rerun("quotient")
    assert pf.commitments[("advice", b2f.halo2_column_index(9))] == honest.commitments[("advice", b2f.halo2_column_index(9))]
    assert pf.evals != honest.evals
    lhs, rhs = pf.identity_sides()
    assert lhs == rhs and lhs != 0
    assert pf.verdict() == "ipa"
