"""b2f_export_fixed_fp_dev and b2f_quotient_gates_dev against the big-integer reference
(tests/quotient_gates_ref.py, which tests/test_quotient_gates_ref.py pins to the oracle's gate code
and by the quotient's degree). Every comparison is bit-exact.

  1  the fixed export: a 3-instance trace, all four forms, every row, row_begin > 0, a padded stride
     whose pattern survives past nrows, against the packed column unpacked on the host;
  2  the gate terms on random columns (random fixed columns too, so no term is trivially zero), every
     row: (k, ext_k) in {(1,2), (2,5), (3,4), (5,7)} in all four forms (11 rot > n_ext in the first
     two: the rotations wrap more than once), (8,11) and (10,12) in the Montgomery form of each field
     (several workgroups, rotations across tile edges and around the end); rows = n_ext + 5 with the
     pad intact; h_in NULL, given, in place; p - 1 and 0 in some cells;
  3  the library's own trace at k = 10, ext_k = 12: the quotient has no coefficient of index
     >= 3n - 3, an altered advice cell in an enabled gate row gives some, sampled rows (within
     11 rot of both ends among them) equal the reference;
  4  the whole numerator at k = 17, ext_k = 19: gates, permutation, lookup into one h in place;
  5  every argument error of the header, nothing launched, then a good call; each call is one timed
     region of its kind.

Needs an MI355X (`-m gpu`)."""
import ctypes

import numpy as np
import pytest

import ntt_ref as nr
import quotient_gates_ref as gr
import quotient_ref as qr

from conftest import random_inputs
from test_gpu_quotient import (PAD, Circuit, _block, _dev, _expect_errors, _first_diff, _gather,
                               _high_coefficients_zero, _host, _limbs4, _omega, _pattern, _random_rows,
                               _stream, _zeta)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ROWS = 1, 3
SMALL = [(1, 2), (2, 5), (3, 4), (5, 7)]


# ---------------------------------------------------------------------------------------------
# 1. the fixed export


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_fixed_export_every_row(engine, form):
    import b2f

    x = random_inputs(3, (0,), 71)
    x["rounds"] = np.asarray([1, 0, 1], dtype=np.uint32)
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    engine.sync(_stream())
    q = batch.fixed.cpu().numpy().view(np.uint32)
    total = len(q)
    assert total == 644 + 228 + 644
    assert all(((q >> g) & 1).any() for g in range(16)) and (q >> 16).any()

    def want(rb, nrows):
        return np.stack([nr.pack(c, form) for c in gr.unpack_fixed(q[rb:rb + nrows])])

    full = want(0, total)
    for rb, nrows, out_rows in ((0, total, total), (0, total, total + 3), (644, 228, 231), (1, 1, 1),
                                (101, 1300, 1301), (total - 1, 1, 4)):
        d_out = _dev(_pattern((17, out_rows, 4)))
        engine.export_fixed_fp_dev(batch.fixed.data_ptr(), total, rb, nrows, form, d_out.data_ptr(), out_rows,
                                   _stream())
        engine.sync(_stream())
        got = _host(d_out)
        assert (got[:, :nrows] == full[:, rb:rb + nrows]).all(), (rb, nrows, out_rows)
        assert (got[:, nrows:] == _pattern((17, out_rows - nrows, 4))).all(), (rb, nrows, out_rows)
    t = batch.export_fixed_fp(engine, form=form)
    engine.sync(_stream())
    assert tuple(t.shape) == (17, total, 4) and (_host(t) == full).all()
    out = _dev(_pattern((17, 300, 4)))
    assert batch.export_fixed_fp(engine, 600, 100, form=form, out=out) is out
    engine.sync(_stream())
    assert (_host(out)[:, :100] == full[:, 600:700]).all() and (_host(out)[:, 100:] == _pattern((17, 200, 4))).all()


# ---------------------------------------------------------------------------------------------
# 2. the gate terms on random columns


class GateProblem:
    """Random extended advice and fixed columns of one (k, ext_k, form), ints and device limbs."""

    def __init__(self, k, ext_k, form, seed):
        self.k, self.ext_k, self.form = k, ext_k, form
        self.p = nr.modulus(form)
        self.n_ext = 1 << ext_k
        self.rows = self.n_ext + PAD
        rng = np.random.default_rng(seed)
        self.adv = [nr.random_elements(rng, self.n_ext, self.p) for _ in range(10)]
        self.fixed = [nr.random_elements(rng, self.n_ext, self.p) for _ in range(17)]
        # the special values ride along
        self.adv[6][0], self.adv[6][1 % self.n_ext], self.adv[8][self.n_ext - 1] = 0, 1, self.p - 1
        self.adv[9][0], self.fixed[3][0], self.fixed[16][self.n_ext - 1] = self.p - 1, self.p - 1, 0
        self.fixed[8][1 % self.n_ext] = 0
        self.h_in = nr.random_elements(rng, self.n_ext, self.p)
        self.h_in[0] = self.p - 1
        self.y = nr.random_elements(rng, 1, self.p)[0]
        self.d_adv, self.d_fixed = _block(self.adv, form, self.rows), _block(self.fixed, form, self.rows)
        self.terms = gr.gate_terms(k, ext_k, self.adv, self.fixed, self.p)
        assert len(self.terms) == 74 and all(any(t) for t in self.terms)

    def h_buffers(self, mode):
        h_in = _block([self.h_in], self.form, self.rows)[0]
        if mode == 0:
            return None, _dev(_pattern((self.rows, 4))), None
        if mode == 1:
            return h_in, _dev(_pattern((self.rows, 4))), self.h_in
        return h_in, h_in, self.h_in

    def run(self, engine, mode):
        h_in, h_out, host_in = self.h_buffers(mode)
        engine.quotient_gates_dev(self.k, self.ext_k, self.d_adv.data_ptr(), self.d_fixed.data_ptr(), self.rows,
                                  self.y, h_in.data_ptr() if h_in is not None else 0, h_out.data_ptr(),
                                  self.form, _stream())
        engine.sync(_stream())
        got = _host(h_out)
        bad = _first_diff(got[:self.n_ext], nr.pack(gr.fold(self.terms, self.y, self.p, host_in), self.form))
        assert bad is None, (self.k, self.ext_k, self.form, mode, "row %d" % bad)
        assert (got[self.n_ext:] == _pattern((PAD, 4))).all(), mode
        if mode == 1:  # the accumulator that came in is as it was
            assert (_host(h_in)[:self.n_ext] == nr.pack(self.h_in, self.form)).all()


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", SMALL)
def test_gate_terms_small(engine, shape, form):
    k, ext_k = shape
    pr = GateProblem(k, ext_k, form, 900 + 10 * k + form)
    before = _host(pr.d_adv).copy(), _host(pr.d_fixed).copy()
    for mode in range(3):
        pr.run(engine, mode)
    assert (_host(pr.d_adv) == before[0]).all() and (_host(pr.d_fixed) == before[1]).all()


@pytest.mark.parametrize("form", [1, 3])
@pytest.mark.parametrize("shape", [(8, 11), (10, 12)])
def test_gate_terms_across_tiles_and_around_the_end(engine, shape, form):
    k, ext_k = shape
    pr = GateProblem(k, ext_k, form, 950 + k + form)
    for mode in ((form + k) % 3, (form + k + 1) % 3):
        pr.run(engine, mode)


def test_tensor_level_call_defaults(engine):
    import torch
    from b2f import B2FError

    form, k, ext_k = 1, 3, 5
    pr = GateProblem(k, ext_k, form, 990)
    want0 = nr.pack(gr.fold(pr.terms, pr.y, pr.p), form)
    h = engine.quotient_gates(k, ext_k, pr.d_adv, pr.d_fixed, pr.y, form=form)
    engine.sync(_stream())
    assert tuple(h.shape) == (pr.n_ext, 4) and (_host(h) == want0).all()
    acc = _block([pr.h_in], form, pr.rows)[0]
    assert engine.quotient_gates(k, ext_k, pr.d_adv, pr.d_fixed, pr.y, h=acc, form=form) is acc  # in place
    engine.sync(_stream())
    assert (_host(acc)[:pr.n_ext] == nr.pack(gr.fold(pr.terms, pr.y, pr.p, pr.h_in), form)).all()
    out = torch.zeros((pr.n_ext, 4), dtype=torch.int64, device="cuda:0")
    assert engine.quotient_gates(k, ext_k, pr.d_adv, pr.d_fixed, pr.y, out=out, form=form) is out
    engine.sync(_stream())
    assert (_host(out) == want0).all()
    for bad in (dict(advice=pr.d_adv[:9]), dict(fixed=pr.d_fixed[:16]), dict(fixed=pr.d_fixed[:, :pr.n_ext].contiguous()),
                dict(advice=pr.d_adv.to(torch.int32)), dict(h=out[:pr.n_ext - 1]), dict(out=out[:, :3])):
        a = dict(dict(advice=pr.d_adv, fixed=pr.d_fixed, h=None, out=None), **bad)
        with pytest.raises(B2FError) as e:
            engine.quotient_gates(k, ext_k, a["advice"], a["fixed"], pr.y, h=a["h"], out=a["out"], form=form)
        assert e.value.code == ERR_ARG, bad


# ---------------------------------------------------------------------------------------------
# 3. the library's own trace


def _near(rows, n_ext, rot):
    return sorted({(i + j * rot) % n_ext for i in rows for j in range(12)})


def _sample(n_ext, rot, count, seed):
    rng = np.random.default_rng(seed)
    edge = {0, 1, rot, 11 * rot - 1, 11 * rot, n_ext - 1, n_ext - rot, n_ext - 11 * rot, n_ext - 11 * rot - 1,
            n_ext - 5 * rot + 1}
    return sorted({i % n_ext for i in edge} | {int(r) for r in rng.integers(0, n_ext, count)})


def test_own_trace_divides_exactly(engine):
    import b2f
    import torch

    form, k, ext_k = 1, 10, 12
    n, n_ext, rot = 1 << k, 1 << ext_k, 4
    p, shift = nr.modulus(form), _zeta(form)
    x = random_inputs(2, (0,), 61)
    x["rounds"] = np.asarray([1, 0], dtype=np.uint32)
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    used = int(batch.offsets_host[-1])
    assert used == 872
    adv = torch.zeros((10, n, 4), dtype=torch.int64, device="cuda:0")
    fixed = torch.zeros((17, n, 4), dtype=torch.int64, device="cuda:0")
    batch.export_fp(engine, 0, used, form=form, out=adv)
    batch.export_fixed_fp(engine, 0, used, form=form, out=fixed)
    adv[:, used:] = _random_rows((10, n - used, 4), 31)  # no gate reads them under an enabled selector
    y = nr.random_elements(np.random.default_rng(32), 1, p)[0]
    adv_e = engine.extend_columns(adv, k, ext_k, shift, form=form)
    fixed_e = engine.extend_columns(fixed, k, ext_k, shift, form=form)
    h = engine.quotient_gates(k, ext_k, adv_e, fixed_e, y, form=form)
    q, zero = _high_coefficients_zero(engine, h, k, ext_k, shift, form)
    assert zero
    rows = _sample(n_ext, rot, 48, 33)
    near = _near(rows, n_ext, rot)
    want = gr.fold(gr.gate_terms(k, ext_k, _gather(adv_e, near, form), _gather(fixed_e, near, form), p, rows=rows),
                   y, p)
    idx = torch.tensor(rows, device="cuda:0")
    assert nr.unpack(_host(h[idx]), form) == want
    assert any(want)
    assert nr.unpack(_host(q[idx]), form) == qr.divide(want, k, ext_k, _omega(form, ext_k), shift, p, rows)
    # one altered advice cell in an enabled gate row: the carry of the first ADD3 block (row 164)
    fx = batch.fixed.cpu().numpy().view(np.uint32)
    assert (int(fx[164]) >> 3) & 1
    bad = adv.clone()
    bad[b2f.halo2_column_index(9), 164, 0] ^= 1
    h = engine.quotient_gates(k, ext_k, engine.extend_columns(bad, k, ext_k, shift, form=form), fixed_e, y, form=form)
    _, zero = _high_coefficients_zero(engine, h, k, ext_k, shift, form)
    assert not zero


# ---------------------------------------------------------------------------------------------
# 4. the whole numerator


def test_gates_permutation_and_lookup_chain_into_one_numerator(engine):
    import torch

    form, k, ext_k = 3, 17, 19
    c = Circuit(engine, random_inputs(25, (12,), 63), k, ext_k, form, 2, 1000)
    assert c.used == 130500 and c.used <= c.usable
    c.permutation_columns()  # c.adv: the advice on the coset, random blinding rows
    c.lookup_columns()
    fixed = torch.zeros((17, c.n, 4), dtype=torch.int64, device="cuda:0")
    c.batch.export_fixed_fp(engine, 0, c.used, form=form, out=fixed)
    fixed_e = c.extend(fixed)
    del fixed
    rot = c.n_ext // c.n
    rows = _sample(c.n_ext, rot, 40, 1001)
    gate_near = _near(rows, c.n_ext, rot)
    gate_terms = gr.gate_terms(k, ext_k, _gather(c.adv, gate_near, form), _gather(fixed_e, gate_near, form), c.p,
                               rows=rows)
    # the gate contribution alone
    h = engine.quotient_gates(k, ext_k, c.adv, fixed_e, c.y, form=form)
    engine.sync(_stream())
    assert c.rows_of(h, rows) == gr.fold(gate_terms, c.y, c.p)
    assert any(any(t) for t in gate_terms)
    _, zero = _high_coefficients_zero(engine, h, k, ext_k, c.shift, form)
    assert zero
    # halo2's order into one accumulator, in place: gates, the permutation, the lookup
    assert c.permutation_h(h=h) is h
    assert c.lookup_h(h=h) is h
    _, zero = _high_coefficients_zero(engine, h, k, ext_k, c.shift, form)
    assert zero
    from test_gpu_quotient import _neighbours

    near = _neighbours(rows, c.n_ext, rot, c.usable)
    want = qr.fold(gate_terms + c.permutation_reference(rows, near) + c.lookup_reference(rows, near), c.y, c.p)
    assert c.rows_of(h, rows) == want


# ---------------------------------------------------------------------------------------------
# 5. errors and timing


def test_argument_errors_then_a_good_call(engine):
    import torch

    form, k, ext_k = 1, 3, 5
    pr = GateProblem(k, ext_k, form, 1100)
    p, n_ext, rows = pr.p, pr.n_ext, pr.rows
    # every block in one buffer, so "unchanged" covers all of them
    sizes = [("adv", 10 * rows), ("fixed", 17 * rows), ("h_in", n_ext), ("h_out", n_ext), ("packed", 8),
             ("exp", 17 * 40)]
    buf = torch.empty((sum(s for _, s in sizes), 4), dtype=torch.int64, device="cuda:0")
    at, off = {}, 0
    for name, size in sizes:
        at[name] = buf.data_ptr() + 32 * off
        if name == "adv":
            buf[off:off + size] = pr.d_adv.reshape(-1, 4)
        elif name == "fixed":
            buf[off:off + size] = pr.d_fixed.reshape(-1, 4)
        elif name == "h_in":
            buf[off:off + size] = _dev(nr.pack(pr.h_in, form))
        else:
            buf[off:off + size] = 0x5A5A5A5A
        off += size
    before = buf.clone()
    s = _stream()

    good = dict(k=k, ext_k=ext_k, d_advice=at["adv"], d_fixed=at["fixed"], rows=rows, y=pr.y, d_h_in=at["h_in"],
                d_h_out=at["h_out"], form=form)

    def gates(**kw):
        a = dict(good, **kw)
        engine.quotient_gates_dev(a["k"], a["ext_k"], a["d_advice"], a["d_fixed"], a["rows"], a["y"], a["d_h_in"],
                                  a["d_h_out"], a["form"], s)

    _expect_errors([
        (ERR_ARG, dict(d_advice=0)), (ERR_ARG, dict(d_fixed=0)), (ERR_ARG, dict(d_h_out=0)),
        (ERR_ARG, dict(d_advice=at["adv"] + 8)), (ERR_ARG, dict(d_fixed=at["fixed"] + 8)),
        (ERR_ARG, dict(d_h_in=at["h_in"] + 8)), (ERR_ARG, dict(d_h_out=at["h_out"] + 8)),
        (ERR_ARG, dict(k=0)), (ERR_ARG, dict(k=ext_k)), (ERR_ARG, dict(k=ext_k + 1)),
        (ERR_ARG, dict(ext_k=29, rows=1 << 29)), (ERR_ARG, dict(form=4)),
        (ERR_ARG, dict(y=p)), (ERR_ARG, dict(y=2**256 - 1)),
        (ERR_ARG, dict(d_h_in=at["h_out"] + 32)),                 # h_in inside h_out, not equal
        (ERR_ARG, dict(d_h_in=at["h_out"] - 32 * (n_ext - 1))),
        (ERR_ARG, dict(d_h_out=at["adv"])),                       # h_out on the first advice row
        (ERR_ARG, dict(d_h_out=at["adv"] + 32 * (10 * rows - 1))),  # ... on the block's last row
        (ERR_ARG, dict(d_h_out=at["fixed"] + 32 * 16 * rows)),    # ... on the k_0 column
        (ERR_ARG, dict(d_h_out=at["fixed"] - 32 * (n_ext - 1))),
        (ERR_ROWS, dict(rows=n_ext - 1)), (ERR_ROWS, dict(rows=0)),
    ], gates)

    good_x = dict(d_fixed=at["packed"], total=64, rb=8, nrows=40, form=form, d_out=at["exp"], out_rows=40)

    def export(**kw):
        a = dict(good_x, **kw)
        engine.export_fixed_fp_dev(a["d_fixed"], a["total"], a["rb"], a["nrows"], a["form"], a["d_out"],
                                   a["out_rows"], s)

    _expect_errors([(ERR_ARG, dict(d_fixed=0)), (ERR_ARG, dict(d_out=0)), (ERR_ARG, dict(form=4)),
                    (ERR_ARG, dict(d_out=at["exp"] + 8)), (ERR_ROWS, dict(rb=65)), (ERR_ROWS, dict(rb=25)),
                    (ERR_ROWS, dict(nrows=57)), (ERR_ROWS, dict(out_rows=39))], export)

    lib, vp = engine.lib, ctypes.c_void_p
    for ctx, yy in ((engine.ctx, None), (None, _limbs4(pr.y))):
        assert lib.b2f_quotient_gates_dev(ctx, k, ext_k, vp(at["adv"]), vp(at["fixed"]), rows, yy, vp(at["h_in"]),
                                          vp(at["h_out"]), form, vp(s)) == ERR_ARG
    assert lib.b2f_export_fixed_fp_dev(None, vp(at["packed"]), 64, 8, 40, form, vp(at["exp"]), 40, vp(s)) == ERR_ARG
    export(nrows=0)  # nothing to do is no error, and writes nothing
    engine.sync(s)
    assert torch.equal(buf, before)  # nothing was launched

    # good calls: each writes its own block and nothing else
    def block(name):
        o = (at[name] - buf.data_ptr()) // 32
        return buf[o:o + dict(sizes)[name]]

    gates()
    engine.sync(s)
    h = gr.fold(pr.terms, pr.y, p, pr.h_in)
    assert _first_diff(_host(block("h_out")), nr.pack(h, form)) is None
    gates(d_h_in=at["h_out"])  # in place, on top
    engine.sync(s)
    assert _first_diff(_host(block("h_out")), nr.pack(gr.fold(pr.terms, pr.y, p, h), form)) is None
    export()
    engine.sync(s)
    packed = _host(block("packed")).view(np.uint32).reshape(-1)  # the fill read as a fixed column
    got = _host(block("exp")).reshape(17, 40, 4)
    assert (got == np.stack([nr.pack(c, form) for c in gr.unpack_fixed(packed[8:48])])).all()
    o = (at["h_out"] - buf.data_ptr()) // 32
    assert torch.equal(buf[:o], before[:o])  # every input block is as it was
    o = (at["packed"] - buf.data_ptr()) // 32
    assert torch.equal(buf[o:o + 8], before[o:o + 8])


def test_each_call_is_one_timed_region(engine):
    import torch

    form, k, ext_k = 3, 5, 7
    pr = GateProblem(k, ext_k, form, 1200)
    s = _stream()
    packed = torch.arange(512, dtype=torch.int32, device="cuda:0")
    out = torch.empty((17, 500, 4), dtype=torch.int64, device="cuda:0")

    def gates():
        pr.run(engine, 1)

    def export():
        engine.export_fixed_fp_dev(packed.data_ptr(), 512, 3, 500, form, out.data_ptr(), 500, s)
        engine.sync(s)

    for call, kind in ((gates, "quotient"), (export, "export")):
        engine.sync(s)
        engine.set_timing(True)
        try:
            call()
            times = engine.kernel_times()
        finally:
            engine.set_timing(False)
        assert times[kind][1] == 1 and times[kind][0] > 0, call.__name__
        assert all(cnt == 0 for name, (_, cnt) in times.items() if name != kind), call.__name__
