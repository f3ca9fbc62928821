"""b2f_ipa_powers_dev / b2f_ipa_round_dev / b2f_ipa_fold_dev (csrc/b2f_ipa.hip) against the
big-integer restatement of tests/ipa_ref.py, bit for bit, on both curves. The generators are known
multiples g_i Gen of the curve's generator, so every expected point is a scalar mod r and one
gen_mul; tests/test_ipa_ref.py ties that restatement to the argument's own identity.

  1  whole openings, k = 1..8, all four forms: after every round L, R, both values and every
     element of the folded p, b, G; the powers call at lengths around a workgroup;
  2  the same openings on the diagnostics library forced all-direct and all-Pippenger;
  3  one long round, len = 2^13 (and 2^11), forms 1 and 3, on the incremental base family;
  4  degenerate points in the generator collapse, mid-wave, with ordinary neighbours, for several u;
  5  degenerate scalars in the round: the product library at two lengths, each path forced;
  6  in place: rows >= half and poisoned guard rows untouched by a round and a fold;
  7  scratch shared with the commitments: round, msm, round; long, short, long;
  8  every refused argument: its code, no timing region, a good call afterwards.

Needs an MI355X (`-m gpu`). No test passes the device anything the host does not check first."""
import os
import random

import numpy as np
import pytest

import ipa_ref as ir
import msm_ref as mr

pytestmark = pytest.mark.gpu

ERR_ARG = 1
POISON = np.uint64(0xfefefefefefefefe)
ALL_DIRECT, ALL_PIPPENGER = "4294967296", "0"


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _sync(eng):
    import torch

    eng.sync(torch.cuda.current_stream().cuda_stream)


def _points(cv, multiples):
    return mr.pack_points(cv, ir.points_of(cv, multiples))


def _round(eng, form, d_p, d_b, d_g, ln):
    """One round on the device -> (lr [2, 8], values [2, 4]) as uint64 arrays."""
    lr, vals = eng.ipa_round(d_p, d_b, d_g, len=ln, form=form)
    _sync(eng)
    return _host(lr), _host(vals)


def _check_round(form, got, l, r, vl, vr, tag):
    cv = mr.curve_of_form(form)
    lr, vals = got
    assert np.array_equal(lr, _points(cv, [l, r])), ("L, R", tag)
    assert np.array_equal(vals, mr.pack_scalars(form, [vl, vr])), ("values", tag)


_opening_inputs = {}


def _opening(form, k):
    """Seeded inputs of a whole opening and its restatement, shared by the tests that run it."""
    cv = mr.curve_of_form(form)
    if (cv, k) not in _opening_inputs:
        r = mr.ORDER[cv]
        rng = random.Random(800 + 10 * k + cv)
        n = 1 << k
        p = [rng.randrange(r) for _ in range(n)]
        x = rng.randrange(1, r)
        us = [rng.randrange(1, r) for _ in range(k)]
        gm, pts = mr.known_bases(form, n)
        _opening_inputs[cv, k] = (p, x, us, pts, ir.opening_known(cv, p, x, gm, us))
    return _opening_inputs[cv, k]


def _run_opening(eng, form, k):
    """The whole loop on the device, every round checked against the restatement. Returns the raw
    outputs of every round, for comparing two engines."""
    cv = mr.curve_of_form(form)
    p, x, us, pts, want = _opening(form, k)
    n = 1 << k
    d_p, d_g = _dev(mr.pack_scalars(form, p)), _dev(mr.pack_points(cv, pts))
    d_b = eng.ipa_powers(x, n, form=form)
    _sync(eng)
    assert np.array_equal(_host(d_b), mr.pack_scalars(form, ir.powers(cv, x, n))), (form, k)
    ln, raw = n, []
    for j, (u, w) in enumerate(zip(us, want)):
        got = _round(eng, form, d_p, d_b, d_g, ln)
        _check_round(form, got, w["l"], w["r"], w["value_l"], w["value_r"], (form, k, j))
        eng.ipa_fold(d_p, d_b, d_g, u, len=ln, form=form)
        _sync(eng)
        half = ln // 2
        hp, hb, hg = _host(d_p), _host(d_b), _host(d_g)
        assert np.array_equal(hp[:half], mr.pack_scalars(form, w["p"])), ("p", form, k, j)
        assert np.array_equal(hb[:half], mr.pack_scalars(form, w["b"])), ("b", form, k, j)
        assert np.array_equal(hg[:half], _points(cv, w["gm"])), ("G", form, k, j)
        raw.append((got[0].copy(), got[1].copy(), hp[:half].copy(), hb[:half].copy(), hg[:half].copy()))
        ln = half
    return raw


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_whole_openings(engine, form):
    for k in range(1, 9):
        _run_opening(engine, form, k)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_powers(engine, form):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(810 + form)
    for ln in (1, 2, 3, 255, 256, 257, 1025):
        for x in (rng.randrange(2, r), 0, 1, r - 1):
            out = engine.ipa_powers(x, ln, form=form)
            _sync(engine)
            assert np.array_equal(_host(out), mr.pack_scalars(form, ir.powers(cv, x, ln))), (form, ln, x)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_both_cross_term_paths(diag_engine, form):
    from b2f import _lib

    assert "B2F_DIAG_IPA_DIRECT" not in os.environ
    runs = {}
    try:
        for forced in (ALL_DIRECT, ALL_PIPPENGER):
            os.environ["B2F_DIAG_IPA_DIRECT"] = forced
            assert _lib.ipa_direct_max_len(diag=True) == int(forced)
            runs[forced] = [_run_opening(diag_engine, form, k) for k in range(1, 9)]
    finally:
        os.environ.pop("B2F_DIAG_IPA_DIRECT", None)
    for a, b in zip(runs[ALL_DIRECT], runs[ALL_PIPPENGER]):
        for ra, rb in zip(a, b):
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))


def _long_round(eng, form, ln, seed, g_checked):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(seed)
    gm, pts = mr.known_bases(form, ln, incremental=True)
    p = [rng.randrange(r) for _ in range(ln)]
    x, u = rng.randrange(1, r), rng.randrange(1, r)
    b = ir.powers(cv, x, ln)
    d_p, d_b, d_g = _dev(mr.pack_scalars(form, p)), _dev(mr.pack_scalars(form, b)), _dev(mr.pack_points(cv, pts))
    l, r_ = ir.round_known(cv, p, gm)
    vl, vr = ir.values(cv, p, b)
    _check_round(form, _round(eng, form, d_p, d_b, d_g, ln), l, r_, vl, vr, (form, ln))
    eng.ipa_fold(d_p, d_b, d_g, u, len=ln, form=form)
    _sync(eng)
    half = ln // 2
    p2, b2 = ir.fold_scalars(cv, p, b, u)
    assert np.array_equal(_host(d_p)[:half], mr.pack_scalars(form, p2))
    assert np.array_equal(_host(d_b)[:half], mr.pack_scalars(form, b2))
    g2 = ir.fold_known(cv, gm, u)
    hg = _host(d_g)
    idx = sorted(g_checked(half, rng))
    assert np.array_equal(hg[idx], _points(cv, [g2[i] for i in idx])), (form, ln)
    # rows from half on are as they were
    assert np.array_equal(_host(d_p)[half:], mr.pack_scalars(form, p[half:]))
    assert np.array_equal(hg[half:], mr.pack_points(cv, pts[half:]))


def _edges_and_seeded(half, rng):
    near = {i for i in range(half) if min(i % 256, 256 - i % 256) <= 2}
    others = [i for i in range(half) if i not in near]
    return near | set(rng.sample(others, 384 - len(near)))


@pytest.mark.parametrize("form", [1, 3])
def test_one_long_round(engine, form):
    _long_round(engine, form, 1 << 13, 820 + form, _edges_and_seeded)
    _long_round(engine, form, 1 << 11, 830 + form, lambda half, rng: set(range(half)))


@pytest.mark.parametrize("form", [1, 3])
def test_degenerate_points_in_the_collapse(engine, form):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(840 + form)
    ln, half = 256, 128
    base_gm, _ = mr.known_bases(form, ln)
    p = [rng.randrange(r) for _ in range(ln)]
    b = [rng.randrange(r) for _ in range(ln)]
    top = 1 << (r.bit_length() - 1)
    for u in (1, 2, r - 1, top, (1 << 200) - 1, top - 1, rng.randrange(1, r)):
        gm = list(base_gm)
        gm[30] = (-u * gm[half + 30]) % r   # G[i] = -[u] G[half+i]: the identity, all zeros
        gm[31] = u * gm[half + 31] % r      # G[i] = [u] G[half+i]: the doubling branch
        gm[half + 33] = 0                   # G[half+i] = (0, 0)
        gm[35] = 0                          # G[i] = (0, 0)
        gm[37] = gm[half + 37] = 0          # both
        gm[96] = (-u * gm[half + 96]) % r   # the same in the second wave
        gm[97] = u * gm[half + 97] % r
        d_p, d_b, d_g = _dev(mr.pack_scalars(form, p)), _dev(mr.pack_scalars(form, b)), _dev(_points(cv, gm))
        engine.ipa_fold(d_p, d_b, d_g, u, len=ln, form=form)
        _sync(engine)
        want = ir.fold_known(cv, gm, u)
        assert want[30] == 0 and want[37] == 0 and want[96] == 0 and want[29] != 0
        hg = _host(d_g)
        assert np.array_equal(hg[:half], _points(cv, want)), (form, u)
        assert not hg[30].any() and not hg[37].any() and hg[29].any() and hg[31].any()
        assert np.array_equal(hg[half:], _points(cv, gm[half:]))
        p2, b2 = ir.fold_scalars(cv, p, b, u)
        assert np.array_equal(_host(d_p)[:half], mr.pack_scalars(form, p2))
        assert np.array_equal(_host(d_b)[:half], mr.pack_scalars(form, b2))


@pytest.mark.parametrize("path,ln", [("product", 64), ("product", 4096), (ALL_DIRECT, 64), (ALL_PIPPENGER, 64)])
@pytest.mark.parametrize("form", [1, 3])
def test_degenerate_scalars_in_the_round(engine, diag_engine, form, path, ln):
    assert "B2F_DIAG_IPA_DIRECT" not in os.environ
    if path == "product":
        return _degenerate_scalars(engine, form, ln)
    try:
        os.environ["B2F_DIAG_IPA_DIRECT"] = path
        _degenerate_scalars(diag_engine, form, ln)
    finally:
        os.environ.pop("B2F_DIAG_IPA_DIRECT", None)


def _degenerate_scalars(engine, form, ln):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(850 + form + ln)
    half = ln // 2
    gm, pts = mr.known_bases(form, ln)
    d_g = _dev(mr.pack_points(cv, pts))
    b = [rng.randrange(1, r) for _ in range(ln)]
    rand = [rng.randrange(1, r) for _ in range(ln)]
    # value_l = 0 mod r with non-zero terms: the last term cancels the others
    bz = list(b)
    rest = sum(rand[half + i] * bz[i] for i in range(half - 1)) % r
    bz[half - 1] = (-rest) * pow(rand[ln - 1], -1, r) % r
    assert bz[half - 1] != 0
    cases = [([0] * ln, b), (rand[:half] + [0] * half, b), (rand, bz), ([r - 1] * ln, b)]
    for n_case, (p, bb) in enumerate(cases):
        d_p, d_b = _dev(mr.pack_scalars(form, p)), _dev(mr.pack_scalars(form, bb))
        l, r_ = ir.round_known(cv, p, gm)
        vl, vr = ir.values(cv, p, bb)
        got = _round(engine, form, d_p, d_b, d_g, ln)
        _check_round(form, got, l, r_, vl, vr, (form, ln, n_case))
        if n_case == 0:
            assert not got[0].any() and not got[1].any()
        if n_case == 1:
            assert not got[0][0].any() and got[0][1].any() and not got[1][0].any()
        if n_case == 2:
            assert vl == 0 and not got[1][0].any() and got[1][1].any()


@pytest.mark.parametrize("form", [1, 3])
def test_in_place_and_untouched(engine, form):
    import torch

    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(860 + form)
    ln, half, guard = 512, 256, 3
    gm, pts = mr.known_bases(form, ln)
    p = [rng.randrange(r) for _ in range(ln)]
    b = [rng.randrange(r) for _ in range(ln)]
    u = rng.randrange(1, r)

    def guarded(arr):
        full = np.full((ln + 2 * guard, arr.shape[1]), POISON, dtype=np.uint64)
        full[guard:guard + ln] = arr
        return _dev(full)

    f_p, f_b, f_g = guarded(mr.pack_scalars(form, p)), guarded(mr.pack_scalars(form, b)), guarded(mr.pack_points(cv, pts))
    d_p, d_b, d_g = (t[guard:guard + ln] for t in (f_p, f_b, f_g))
    before = [t.clone() for t in (f_p, f_b, f_g)]
    l, r_ = ir.round_known(cv, p, gm)
    vl, vr = ir.values(cv, p, b)
    _check_round(form, _round(engine, form, d_p, d_b, d_g, ln), l, r_, vl, vr, form)
    assert all(torch.equal(a, c) for a, c in zip(before, (f_p, f_b, f_g))), "the round wrote to an input"
    engine.ipa_fold(d_p, d_b, d_g, u, len=ln, form=form)
    _sync(engine)
    p2, b2 = ir.fold_scalars(cv, p, b, u)
    for full, was, lo in ((f_p, before[0], mr.pack_scalars(form, p2)), (f_b, before[1], mr.pack_scalars(form, b2)),
                          (f_g, before[2], _points(cv, ir.fold_known(cv, gm, u)))):
        h, w = _host(full), _host(was)
        assert np.array_equal(h[guard:guard + half], lo)
        assert np.array_equal(h[guard + half:], w[guard + half:]), "rows >= half or the guard rows below changed"
        assert np.array_equal(h[:guard], w[:guard]) and (h[:guard] == POISON).all()
        assert (h[guard + ln:] == POISON).all()


@pytest.mark.parametrize("form", [1, 3])
def test_scratch_shared_with_the_commitments(form):
    import b2f

    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(870 + form)
    long_ln, short_ln = 1 << 12, 32
    gm, pts = mr.known_bases(form, long_ln)
    eng = b2f.Engine(0)
    try:
        d_g = _dev(mr.pack_points(cv, pts))
        vec = {}
        for ln in (long_ln, short_ln):
            p = [rng.randrange(r) for _ in range(ln)]
            b = [rng.randrange(r) for _ in range(ln)]
            vec[ln] = (p, b, _dev(mr.pack_scalars(form, p)), _dev(mr.pack_scalars(form, b)))

        def run(ln):
            p, b, d_p, d_b = vec[ln]
            got = _round(eng, form, d_p, d_b, d_g, ln)
            l, r_ = ir.round_known(cv, p, gm[:ln])
            _check_round(form, got, l, r_, *ir.values(cv, p, b), (form, ln))
            return got

        first = run(long_ln)
        # an unrelated commitment on the same context, larger than the round's own pass
        cols = [[rng.randrange(r) for _ in range(3000)] for _ in range(5)]
        sc = np.stack([mr.pack_scalars(form, c) for c in cols])
        out = eng.msm(_dev(sc), d_g, len=3000, form=form)
        _sync(eng)
        assert mr.unpack_points(cv, _host(out)) == [mr.expected_msm(form, c, gm[:3000]) for c in cols]
        again = run(long_ln)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        run(short_ln)
        third = run(long_ln)
        assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1])
    finally:
        eng.close()


def test_refused_arguments(engine):
    import torch

    from b2f import B2FError

    form, cv, ln = 1, 0, 16
    r = mr.ORDER[cv]
    rng = random.Random(880)
    gm, pts = mr.known_bases(form, ln)
    p = [rng.randrange(r) for _ in range(ln)]
    x, u = rng.randrange(1, r), rng.randrange(1, r)
    b = ir.powers(cv, x, ln)
    d_p0, d_g0 = _dev(mr.pack_scalars(form, p)), _dev(mr.pack_points(cv, pts))
    d_p, d_g = d_p0.clone(), d_g0.clone()
    d_b = torch.zeros((ln, 4), dtype=torch.int64, device="cuda:0")
    d_lr = torch.zeros((2, 8), dtype=torch.int64, device="cuda:0")
    d_v = torch.zeros((2, 4), dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    P, B, G, LR, V = (t.data_ptr() for t in (d_p, d_b, d_g, d_lr, d_v))
    l, r_ = ir.round_known(cv, p, gm)
    vl, vr = ir.values(cv, p, b)
    p2, b2 = ir.fold_scalars(cv, p, b, u)

    def good():
        d_p.copy_(d_p0)
        d_g.copy_(d_g0)
        d_lr.zero_()
        engine.ipa_powers_dev(x, ln, form, B, s)
        engine.ipa_round_dev(P, B, G, ln, form, LR, V, s)
        engine.ipa_fold_dev(P, B, G, ln, u, form, s)
        engine.sync(s)
        _check_round(form, (_host(d_lr), _host(d_v)), l, r_, vl, vr, "good")
        assert np.array_equal(_host(d_p)[:ln // 2], mr.pack_scalars(form, p2))
        assert np.array_equal(_host(d_b)[:ln // 2], mr.pack_scalars(form, b2))
        assert np.array_equal(_host(d_g)[:ln // 2], _points(cv, ir.fold_known(cv, gm, u)))

    good()
    big = 1 << 29
    refused = [
        (engine.ipa_powers_dev, (x, ln, form, 0)), (engine.ipa_powers_dev, (x, ln, form, B + 8)),
        (engine.ipa_powers_dev, (x, ln, 4, B)), (engine.ipa_powers_dev, (x, 0, form, B)),
        (engine.ipa_powers_dev, (x, (1 << 28) + 1, form, B)), (engine.ipa_powers_dev, (r, ln, form, B)),
        (engine.ipa_powers_dev, ((1 << 256) - 1, ln, form, B)),
    ]
    for bad in ((0, B, G, ln, form, LR, V), (P, 0, G, ln, form, LR, V), (P, B, 0, ln, form, LR, V),
                (P, B, G, ln, form, 0, V), (P, B, G, ln, form, LR, 0),
                (P + 8, B, G, ln, form, LR, V), (P, B + 8, G, ln, form, LR, V), (P, B, G + 8, ln, form, LR, V),
                (P, B, G, ln, form, LR + 8, V), (P, B, G, ln, form, LR, V + 8),
                (P, B, G, ln, 4, LR, V),
                (P, B, G, 0, form, LR, V), (P, B, G, 1, form, LR, V), (P, B, G, 3, form, LR, V),
                (P, B, G, 12, form, LR, V), (P, B, G, big, form, LR, V),
                (P, B, G, ln, form, P, V), (P, B, G, ln, form, G + 64 * (ln - 1), V),   # L, R on an input
                (P, B, G, ln, form, LR, B + 32 * (ln - 2)), (P, B, G, ln, form, LR, LR + 64),  # the values on b, on R
                (P, P + 32, G, ln // 2, form, LR, V),  # b inside p
                (P, B, P, ln // 4, form, LR, V)):                   # G on p
        refused.append((engine.ipa_round_dev, bad))
    for bad in ((0, B, G, ln, u, form), (P, 0, G, ln, u, form), (P, B, 0, ln, u, form),
                (P + 8, B, G, ln, u, form), (P, B + 8, G, ln, u, form), (P, B, G + 8, ln, u, form),
                (P, B, G, ln, u, 4), (P, B, G, 0, u, form), (P, B, G, 1, u, form), (P, B, G, 6, u, form),
                (P, B, G, big, u, form), (P, B, G, ln, 0, form), (P, B, G, ln, r, form),
                (P, B, G, ln, r + 5, form), (P, P + 32, G, 2, u, form), (P, B, B, ln // 2, u, form)):
        refused.append((engine.ipa_fold_dev, bad))
    for fn, args in refused:
        engine.set_timing(True)
        with pytest.raises(B2FError) as e:
            fn(*args, s)
        assert e.value.code == ERR_ARG, (fn.__name__, args)
        times = engine.kernel_times()
        engine.set_timing(False)
        assert all(v[1] == 0 for v in times.values()), (fn.__name__, args)
        good()
    # each good call is one region of the quotient kind
    engine.set_timing(True)
    engine.ipa_powers_dev(x, ln, form, B, s)
    engine.ipa_round_dev(P, B, G, ln, form, LR, V, s)
    engine.ipa_fold_dev(P, B, G, ln, u, form, s)
    times = engine.kernel_times()
    engine.set_timing(False)
    assert times["quotient"][1] == 3 and times["quotient"][0] > 0
    assert all(v[1] == 0 for k, v in times.items() if k != "quotient")
