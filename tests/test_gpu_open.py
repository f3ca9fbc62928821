"""The evaluation / opening calls on the device (b2f_poly_eval_dev, b2f_poly_combine_dev,
b2f_kate_divide_dev) against tests/open_ref.py, bit for bit: every length around the tile (1,024
coefficients, a power of two) and the wave, all four forms, the pad rows, the multiopen field side
composed from the three calls, and the chip's own quotient evaluated at a point."""
import ctypes

import numpy as np
import pytest

import ntt_ref as nr
import open_ref as orf
import quotient_gates_ref as gr

from conftest import random_inputs
from test_gpu_quotient import _block, _dev, _expect_errors, _host, _pattern, _random_rows, _stream, _zeta

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ROWS = 1, 3
SMALL = list(range(1, 131)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 3 * 4096 + 1, 2**16 + 1]
PAD = 5


def _lengths(form):
    return SMALL if form in (1, 3) else [n for n in SMALL if n <= 257]


_POOL = {}


def _pool(form):
    """Random elements shared by the small-length tests of one field, generated once."""
    p = nr.modulus(form)
    if p not in _POOL:
        _POOL[p] = nr.random_elements(np.random.default_rng(900 + (form >> 1)), max(SMALL) + 70000, p)
    return _POOL[p]


def _columns(form, n, count):
    """`count` columns of n coefficients with 0 and p - 1 in some cells."""
    p, pool = nr.modulus(form), _pool(form)
    cols = [list(pool[c * 6151 + (n % 7): c * 6151 + (n % 7) + n]) for c in range(count)]
    cols[0][0] = 0
    cols[1][-1] = p - 1
    cols[count - 1][n // 2] = 0
    cols[count - 1][-1] = p - 1 if n > 1 else cols[count - 1][-1]
    return cols


def _points(form):
    """0, 1, p - 1 and nine random points."""
    p = nr.modulus(form)
    return [0, 1, p - 1] + _pool(form)[-9:]


def _unpack(t, form):
    return nr.unpack(_host(t).reshape(-1, 4), form)


# ---------------------------------------------------------------------------------------------
# 1, 2. evaluation

QUERIES = [(2, 3), (0, 4), (0, 0), (0, 1), (2, 0), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 9),
           (0, 10), (0, 11), (2, 3), (2, 2), (0, 0)]  # column 1 unqueried, twelve points on column 0, repeats


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_evaluation_small(engine, form):
    import torch

    p, pts = nr.modulus(form), _points(form)
    s = _stream()
    for n in _lengths(form):
        cols = _columns(form, n, 3)
        block = _block(cols, form, n + PAD)
        before = block.clone()
        got = engine.poly_eval(block, pts, QUERIES, len=n, form=form)
        engine.sync(s)
        want = [orf.eval(cols[c], pts[q], p) for c, q in QUERIES]
        assert _unpack(got, form) == want, n
        assert torch.equal(block, before), n


@pytest.mark.parametrize("shape", [(2**18 + 3, 2, 3, 1), (2**12, 70, 1, 3)])
def test_evaluation_many_tiles_and_many_columns(engine, shape):
    import torch

    n, n_cols, n_pts, form = shape
    p = nr.modulus(form)
    block = _random_rows((n_cols, n + PAD, 4), 910 + n_cols)
    before = block.clone()
    pts = nr.random_elements(np.random.default_rng(911), n_pts, p)
    queries = [(c, q) for q in range(n_pts) for c in reversed(range(n_cols))]
    got = engine.poly_eval(block, pts, queries, len=n, form=form)
    engine.sync(_stream())
    cols = [_unpack(block[c, :n], form) for c in range(n_cols)]
    assert _unpack(got, form) == [orf.eval(cols[c], pts[q], p) for c, q in queries]
    assert torch.equal(block, before)


# ---------------------------------------------------------------------------------------------
# 3. combine


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_combine_small(engine, form):
    import torch

    p = nr.modulus(form)
    r = _pool(form)[-8:]
    combos = [[], [(2, 1)],
              [(0, r[0]), (1, 0), (3, p - 1), (0, r[1]), (2, r[2]), (3, r[3]), (1, 1), (0, p - 1)]]
    s = _stream()
    for n in _lengths(form):
        cols = _columns(form, n, 4)
        block = _block(cols, form, n + 2)
        before = block.clone()
        out = _dev(_pattern((3, n + PAD, 4)))
        engine.poly_combine(block, combos, len=n, form=form, out=out)
        engine.sync(s)
        for o, terms in enumerate(combos):
            assert _unpack(out[o, :n], form) == orf.combine(cols, terms, n, p), (n, o)
        assert (_host(out[:, n:]) == _pattern((3, PAD, 4))).all(), n
        assert torch.equal(block, before), n
    # the default output: [n_out, len, 4]
    got = engine.poly_combine(block, combos[1:], form=form)
    engine.sync(s)
    assert tuple(got.shape) == (2, block.shape[1], 4)


# ---------------------------------------------------------------------------------------------
# 4, 5. division


def _chains(form, n):
    """Point lists with m = 0, 1, 2 (a repeated point), 3, 12, n and n + 1, mixed in one call; the
    single division is by 0, 1, p - 1 or a random point in turn with n (by each of them at every
    small n, where three more columns cost nothing)."""
    p, r = nr.modulus(form), _pool(form)
    special = [0, 1, p - 1, r[5]]
    twelve = [r[10], 0, r[11], 1, r[12], p - 1, r[13], r[14], r[10], r[15], r[16], r[17]]
    chains = [[], [special[n % 4]], [r[6], r[6]], [0, 1, p - 1], twelve, r[100:100 + n], r[200:201 + n]]
    if n <= 257:
        chains += [[special[(n + 1) % 4]], [special[(n + 2) % 4]], [special[(n + 3) % 4]]]
    return chains


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_division_every_row(engine, form):
    import torch

    p = nr.modulus(form)
    s = _stream()
    for n in _lengths(form):
        chains = _chains(form, n)
        cols = _columns(form, n, len(chains))
        block = _block(cols, form, n + 3)
        before = block.clone()
        out = _dev(_pattern((len(chains), n + PAD, 4)))
        engine.kate_divide(block, chains, len=n, form=form, out=out)
        engine.sync(s)
        for c, pts in enumerate(chains):
            got = _unpack(out[c, :n], form)
            assert got == orf.divide_chain(cols[c], pts, p), (n, c)
            m = min(len(pts), n)
            assert got[n - m:] == [0] * m
        assert (_host(out[:, n:]) == _pattern((len(chains), PAD, 4))).all(), n
        assert torch.equal(block, before), n


@pytest.mark.parametrize("shape", [(2**18 + 3, (1, 3)), (2**20 + 3, (1,))])
def test_division_many_tiles(engine, shape):
    import torch

    n, ms = shape
    form = 1
    p = nr.modulus(form)
    block = _random_rows((len(ms), n + 2, 4), 920)
    before = block.clone()
    pts = nr.random_elements(np.random.default_rng(921), sum(ms), p)
    chains, at = [], 0
    for m in ms:
        chains.append(pts[at:at + m])
        at += m
    out = _dev(_pattern((len(ms), n + PAD, 4)))
    engine.kate_divide(block, chains, len=n, form=form, out=out)
    engine.sync(_stream())
    for c, chain in enumerate(chains):
        got = _unpack(out[c, :n], form)
        assert got == orf.divide_chain(_unpack(block[c, :n], form), chain, p), c
        assert got[n - len(chain):] == [0] * len(chain)
    assert (_host(out[:, n:]) == _pattern((len(ms), PAD, 4))).all()
    assert torch.equal(block, before)


@pytest.mark.parametrize("form", [1, 3])
def test_division_against_evaluation(engine, form):
    """a_0 + z q_0 = p(z): the division's carries and the evaluation's sums are the same tile values."""
    n = 4097
    p = nr.modulus(form)
    cols = _columns(form, n, 2)
    block = _block(cols, form, n)
    zs = _pool(form)[300:302]
    q = engine.kate_divide(block, [[zs[0]], [zs[1]]], form=form)
    ev = engine.poly_eval(block, zs, [(0, 0), (1, 1)], form=form)
    engine.sync(_stream())
    q0 = _unpack(q[:, 0], form)
    assert _unpack(ev, form) == [(cols[c][0] + zs[c] * q0[c]) % p for c in range(2)]


# ---------------------------------------------------------------------------------------------
# 6. the multiopen field side through the three calls


@pytest.mark.parametrize("form", [1, 3])
def test_multiopen_field_side(engine, form):
    import torch
    from b2f import field

    k, n = 8, 256
    p, f = nr.modulus(form), field.of_form(form)
    rng = np.random.default_rng(930 + form)
    polys = [nr.random_elements(rng, n, p) for _ in range(12)]
    x, x1, x2, x3, x4 = nr.random_elements(rng, 5, p)
    sets = [(field.rotated_points(f, x, k, [0]), [0, 1, 2, 3]),
            (field.rotated_points(f, x, k, [0, 1]), [4, 5, 6]),
            (field.rotated_points(f, x, k, [0, 1, -1]), [7, 8, 9]),
            (field.rotated_points(f, x, k, range(12)), [10, 11])]
    want = orf.multiopen_field_side(polys, sets, x1, x2, x3, x4, p)
    s = _stream()

    # the evaluations of every polynomial at every point of its set, one call
    points = sorted({z for pts, _ in sets for z in pts})
    queries = [(m, points.index(z)) for pts, members in sets for m in members for z in pts]
    cols = _block(polys, form, n)
    ev = engine.poly_eval(cols, points, queries, form=form)
    engine.sync(s)
    ev = dict(zip(queries, _unpack(ev, form)))
    # the x_1 fold of the evaluations and their interpolation r(X): a few elements, on the host
    r_polys = []
    for pts, members in sets:
        folded = [0] * len(pts)
        for m in members:
            folded = [(e * x1 + ev[(m, points.index(z))]) % p for e, z in zip(folded, pts)]
        r_polys.append(orf.interpolate(pts, folded, p))
    assert r_polys == want["r_polys"]
    # q_set = the x_1 fold of the set's polynomials, and q_set - r_set, one call
    both = torch.cat([cols, _block([r + [0] * (n - len(r)) for r in r_polys], form, n)])
    fold = [[(m, pow(x1, len(members) - 1 - i, p)) for i, m in enumerate(members)] for _, members in sets]
    diff = [terms + [(12 + i, p - 1)] for i, terms in enumerate(fold)]
    qd = engine.poly_combine(both, fold + diff, form=form)
    # the division chains, the x_2 fold, the evaluations at x_3, the x_4 fold
    quo = engine.kate_divide(qd[4:].contiguous(), [pts for pts, _ in sets], form=form)
    f_poly = engine.poly_combine(quo, [[(i, pow(x2, 3 - i, p)) for i in range(4)]], form=form)
    q_at_x3 = engine.poly_eval(qd[:4].contiguous(), [x3], [(i, 0) for i in range(4)], form=form)
    last = torch.cat([qd[:4], f_poly])
    final = engine.poly_combine(last, [[(4, pow(x4, 4, p))] + [(i, pow(x4, 3 - i, p)) for i in range(4)]], form=form)
    engine.sync(s)
    for i in range(4):
        assert _unpack(qd[i], form) == want["q_polys"][i], i
        assert _unpack(quo[i], form) == want["quotients"][i], i
    assert _unpack(f_poly[0], form) == want["f_poly"]
    assert _unpack(q_at_x3, form) == want["q_at_x3"]
    assert _unpack(final[0], form) == want["final_poly"]


# ---------------------------------------------------------------------------------------------
# 7. the chip's own quotient at a point


def test_own_quotient_at_a_point(engine):
    import b2f
    import torch
    from b2f import field

    form, k, ext_k = 1, 10, 12
    n = 1 << k
    p, shift, f = nr.modulus(form), _zeta(form), field.of_form(form)
    x = random_inputs(2, (0,), 61)
    x["rounds"] = np.asarray([1, 0], dtype=np.uint32)
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    used = int(batch.offsets_host[-1])
    adv = torch.zeros((10, n, 4), dtype=torch.int64, device="cuda:0")
    fixed = torch.zeros((17, n, 4), dtype=torch.int64, device="cuda:0")
    batch.export_fp(engine, 0, used, form=form, out=adv)
    batch.export_fixed_fp(engine, 0, used, form=form, out=fixed)
    adv[:, used:] = _random_rows((10, n - used, 4), 31)
    rng = np.random.default_rng(940)
    y, xp = nr.random_elements(rng, 2, p)
    queries = [tuple(int(v) for v in row) for row in b2f.gate_queries()]
    points = field.rotated_points(f, xp, k, range(12))
    s = _stream()
    fixed_c = engine.ntt_columns(fixed, k, inverse=True, form=form)
    fixed_e = engine.ntt_columns(fixed_c, ext_k, shift=shift, in_len=n, form=form)
    fixed_x = _unpack(engine.poly_eval(fixed_c, [xp], [(g, 0) for g in range(17)], form=form), form)

    def sides(advice):
        adv_c = engine.ntt_columns(advice, k, inverse=True, form=form)
        adv_e = engine.ntt_columns(adv_c, ext_k, shift=shift, in_len=n, form=form)
        h = engine.quotient_gates(k, ext_k, adv_e, fixed_e, y, form=form)
        h = engine.quotient_divide(k, ext_k, shift, h, form=form)
        coeff = engine.ntt_columns(h[None], ext_k, inverse=True, shift=shift, form=form)
        pieces = coeff.reshape(4, n, 4)  # the h pieces: columns of stride n
        h_x = _unpack(engine.poly_eval(pieces, [xp], [(i, 0) for i in range(4)], form=form), form)
        a_x = dict(zip(queries, _unpack(engine.poly_eval(adv_c, points, queries, form=form), form)))
        engine.sync(s)
        xn = pow(xp, n, p)
        left = (xn - 1) * sum(pow(xn, i, p) * v for i, v in enumerate(h_x)) % p
        right = 0
        for g in range(16):
            polys = [a_x[(gr.HALO2[1], 0)] - fixed_x[16]] if g == 14 else gr.GATES[g](lambda c, j: a_x[(gr.HALO2[c], j)])
            for poly in polys:
                right = (right * y + fixed_x[g] * poly) % p
        return left, right

    left, right = sides(adv)
    assert left == right and left != 0
    bad = adv.clone()
    bad[b2f.halo2_column_index(9), 164, 0] ^= 1  # the carry of the first ADD3 block, as in the quotient test
    left, right = sides(bad)
    assert left != right


# ---------------------------------------------------------------------------------------------
# 8. errors


def _raw(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).copy()


def test_argument_errors_then_good_calls(engine):
    import torch

    form, n, rows = 1, 300, 304
    p = nr.modulus(form)
    cols = _columns(form, n, 3)
    sizes = [("cols", 3 * rows), ("out", 3 * rows), ("ev", 8)]
    buf = torch.empty((sum(sz for _, sz in sizes), 4), dtype=torch.int64, device="cuda:0")
    buf[:] = 0x5A5A5A5A
    buf[:3 * rows] = _block(cols, form, rows).reshape(-1, 4)
    at, off = {}, 0
    for name, sz in sizes:
        at[name] = buf.data_ptr() + 32 * off
        off += sz
    before = buf.clone()
    s = _stream()
    z = _pool(form)[400:403]

    good_e = dict(d_cols=at["cols"], rows=rows, n=n, n_cols=3, points=z, queries=[(0, 0), (2, 1)], form=form,
                  d_out=at["ev"])

    def ev(**kw):
        a = dict(good_e, **kw)
        engine.poly_eval_dev(a["d_cols"], a["rows"], a["n"], a["n_cols"], a["points"], a["queries"], a["form"],
                             a["d_out"], s)

    _expect_errors([
        (ERR_ARG, dict(d_cols=0)), (ERR_ARG, dict(d_out=0)), (ERR_ARG, dict(d_cols=at["cols"] + 8)),
        (ERR_ARG, dict(d_out=at["ev"] + 8)), (ERR_ARG, dict(form=4)), (ERR_ARG, dict(n=0)), (ERR_ARG, dict(n_cols=0)),
        (ERR_ARG, dict(queries=[])), (ERR_ARG, dict(points=[])), (ERR_ARG, dict(queries=[(0, 0), (3, 1)])),
        (ERR_ARG, dict(queries=[(0, 3)])), (ERR_ARG, dict(points=[z[0], p, z[2]])),
        (ERR_ARG, dict(points=[2**256 - 1])), (ERR_ARG, dict(d_out=at["cols"])),
        (ERR_ARG, dict(d_out=at["cols"] + 32 * (3 * rows - 1))), (ERR_ARG, dict(d_out=at["cols"] - 32)),
        (ERR_ROWS, dict(n=rows + 1)), (ERR_ROWS, dict(rows=n - 1)),
    ], ev)

    good_c = dict(d_cols=at["cols"], rows=rows, n=n, n_cols=3, combos=[[(0, 3), (2, z[0])], []], form=form,
                  d_out=at["out"], out_rows=rows)

    def comb(**kw):
        a = dict(good_c, **kw)
        engine.poly_combine_dev(a["d_cols"], a["rows"], a["n"], a["n_cols"], a["combos"], a["form"], a["d_out"],
                                a["out_rows"], s)

    _expect_errors([
        (ERR_ARG, dict(d_cols=0)), (ERR_ARG, dict(d_out=0)), (ERR_ARG, dict(d_cols=at["cols"] + 8)),
        (ERR_ARG, dict(d_out=at["out"] + 8)), (ERR_ARG, dict(form=4)), (ERR_ARG, dict(n=0)), (ERR_ARG, dict(n_cols=0)),
        (ERR_ARG, dict(combos=[])), (ERR_ARG, dict(combos=[[(3, 1)]])), (ERR_ARG, dict(combos=[[], [(0, p)]])),
        (ERR_ARG, dict(d_out=at["cols"] + 32 * (3 * rows - 1))), (ERR_ARG, dict(d_out=at["cols"] - 32 * (rows + n - 1))),
        (ERR_ROWS, dict(n=rows + 1)), (ERR_ROWS, dict(out_rows=n - 1)),
    ], comb)

    good_k = dict(d_cols=at["cols"], rows=rows, n=n, n_cols=3, chains=[[z[0]], [], [z[1], z[2]]], form=form,
                  d_out=at["out"], out_rows=rows)

    def kate(**kw):
        a = dict(good_k, **kw)
        engine.kate_divide_dev(a["d_cols"], a["rows"], a["n"], a["n_cols"], a["chains"], a["form"], a["d_out"],
                               a["out_rows"], s)

    _expect_errors([
        (ERR_ARG, dict(d_cols=0)), (ERR_ARG, dict(d_out=0)), (ERR_ARG, dict(d_cols=at["cols"] + 8)),
        (ERR_ARG, dict(d_out=at["out"] + 8)), (ERR_ARG, dict(form=4)), (ERR_ARG, dict(n=0)),
        (ERR_ARG, dict(n_cols=0, chains=[])), (ERR_ARG, dict(chains=[[z[0]], [p], []])),
        (ERR_ARG, dict(d_out=at["cols"] + 32 * (3 * rows - 1))), (ERR_ARG, dict(d_out=at["cols"] - 32 * (2 * rows + n - 1))),
        (ERR_ROWS, dict(n=rows + 1)), (ERR_ROWS, dict(out_rows=n - 1)),
    ], kate)

    # what the helpers cannot express: null host arrays, an h_first that decreases or starts past 0
    lib, vp = engine.lib, ctypes.c_void_p
    pts, qs = _raw(z), np.array([0, 0, 2, 1], dtype=np.uint32)
    first_bad, first_off = np.array([0, 2, 1, 3], dtype=np.uint32), np.array([1, 2, 3, 3], dtype=np.uint32)
    first_ok, col = np.array([0, 1, 2, 3], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint32)
    P = lambda a: vp(a.ctypes.data)  # noqa: E731
    assert lib.b2f_poly_eval_dev(engine.ctx, vp(at["cols"]), rows, n, 3, None, 3, P(qs), 2, form, vp(at["ev"]),
                                 vp(s)) == ERR_ARG
    assert lib.b2f_poly_eval_dev(engine.ctx, vp(at["cols"]), rows, n, 3, P(pts), 3, None, 2, form, vp(at["ev"]),
                                 vp(s)) == ERR_ARG
    assert lib.b2f_poly_eval_dev(None, vp(at["cols"]), rows, n, 3, P(pts), 3, P(qs), 2, form, vp(at["ev"]),
                                 vp(s)) == ERR_ARG
    for first in (first_bad, first_off, None):
        f = P(first) if first is not None else None
        assert lib.b2f_poly_combine_dev(engine.ctx, vp(at["cols"]), rows, n, 3, f, P(col), P(pts), 3, form,
                                        vp(at["out"]), rows, vp(s)) == ERR_ARG
        assert lib.b2f_kate_divide_dev(engine.ctx, vp(at["cols"]), rows, n, 3, f, P(pts), form, vp(at["out"]), rows,
                                       vp(s)) == ERR_ARG
    assert lib.b2f_poly_combine_dev(engine.ctx, vp(at["cols"]), rows, n, 3, P(first_ok), None, P(pts), 3, form,
                                    vp(at["out"]), rows, vp(s)) == ERR_ARG
    assert lib.b2f_kate_divide_dev(engine.ctx, vp(at["cols"]), rows, n, 3, P(first_ok), None, form, vp(at["out"]),
                                   rows, vp(s)) == ERR_ARG
    assert lib.b2f_kate_divide_dev(None, vp(at["cols"]), rows, n, 3, P(first_ok), P(pts), form, vp(at["out"]), rows,
                                   vp(s)) == ERR_ARG
    engine.sync(s)
    assert torch.equal(buf, before)  # nothing was launched

    out = buf[3 * rows:6 * rows].reshape(3, rows, 4)
    ev()
    engine.sync(s)
    assert _unpack(buf[6 * rows:6 * rows + 2], form) == [orf.eval(cols[0], z[0], p), orf.eval(cols[2], z[1], p)]
    comb()
    engine.sync(s)
    assert _unpack(out[0, :n], form) == orf.combine(cols, good_c["combos"][0], n, p)
    assert _unpack(out[1, :n], form) == [0] * n
    kate()
    engine.sync(s)
    for c, chain in enumerate(good_k["chains"]):
        assert _unpack(out[c, :n], form) == orf.divide_chain(cols[c], chain, p)
    assert torch.equal(buf[:3 * rows], before[:3 * rows])            # the inputs
    assert torch.equal(out[:, n:], before[3 * rows:6 * rows].reshape(3, rows, 4)[:, n:])  # the output pads
    assert torch.equal(buf[6 * rows + 2:], before[6 * rows + 2:])


# ---------------------------------------------------------------------------------------------
# 9. timing


def test_each_call_is_one_quotient_region(engine):
    form, n = 3, 2500
    cols = _block(_columns(form, n, 3), form, n)
    z = _pool(form)[500:503]
    s = _stream()
    calls = [lambda: engine.poly_eval(cols, z, [(0, 0), (1, 2), (0, 1)], form=form),
             lambda: engine.poly_combine(cols, [[(0, 2), (1, z[0])]], form=form),
             lambda: engine.kate_divide(cols, [[z[0]], z, []], form=form)]
    for i, call in enumerate(calls):
        engine.sync(s)
        engine.set_timing(True)
        try:
            call()
            engine.sync(s)
            times = engine.kernel_times()
        finally:
            engine.set_timing(False)
        assert len(times) == 10
        assert times["quotient"][1] == 1 and times["quotient"][0] > 0, i
        assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "quotient"), i
