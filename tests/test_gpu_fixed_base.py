"""b2f_fixed_base_mul_dev (csrc/b2f_fixed_base.hip: out[i] = [s_i] B) and Engine.kzg_setup on the
MI355X, bit for bit against tests/fixed_base_ref.py, on both curves. Bases are known multiples of
the generator, so every expectation is one fixed-base multiple in big integers.

  1  lengths 1, 63, 64, 65, 257, 4,099: one lane, the wave boundary, several workgroups, a ragged
     tail;
  2  the four forms at len 257: canonical and Montgomery scalars of the same values give the same
     points;
  3  scalars that steer the recoding, for the digit width the plan reports: 0, 1, r - 1, r - 2,
     (r - 1) / 2, 2^254 -+ 1 where below r, every digit 2^(c-1) / 2^(c-1) - 1 / 2^(c-1) + 1
     (reduced), one non-zero digit (+1, -1, the largest entry) in each window, 2^(w c) and
     2^(w c) - 1 for every window;
  4  the additions where the accumulator meets the addend: a reduced scalar whose last addition is
     P + P, and the unreduced scalar r (canonical forms only: it has no Montgomery form), the one
     input whose accumulation ends in P - P. For a reduced scalar and a base of prime order r a
     partial sum that is 0 mod r would have to be 0, so no reduced scalar reaches P - P; the
     reference asserts both events before the device is asked;
  5  bases: the generator, a random multiple, [r - 1] G, the identity (all zeros out), and an
     off-curve point (the call returns, the sync is B2F_OK or B2F_ERR_CHECK, nothing outside d_out
     changes);
  6  the table cache: A, B, A; five distinct bases (one more than the cache holds), then the first;
  7  a repeated base: every call is one B2F_KERNEL_QUOTIENT region whether it builds a table or
     not, so the region count cannot show that the second call launches no build. That is checked
     by timing in tools/bench_fixed_base.py only (first call against steady state); here the
     repeat is checked for its result and its one region;
  8  kzg_setup(10, tau): g[i] == [tau^i] G for all 1,024 points, g_lagrange against
     group_ntt_ref on a sample;
  9  the defining property on the device at k = 10: msm(col, g) == fixed_base_mul([col(tau)]);
 10  the call on a caller's non-blocking stream queued behind an in-flight MSM, the table of a new
     base rebuilt in stream order;
 11  d_scalars and d_out at 16-byte-only addresses carved from a poisoned arena, guards intact;
 12  every refused argument is B2F_ERR_ARG, launches nothing, and the next good call is right.

Needs an MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import fixed_base_ref as fb
import group_ntt_ref as gn
import msm_ref as mr
import ntt_ref as nr

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_CHECK = 0, 1, 8
LENGTHS = [1, 63, 64, 65, 257, 4099]
BASE_MULTIPLE = (0x1f3a5c7e9b2d4f60718293a4b5c6d7e8f9012345678abcdef0, 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da5)


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _sync(eng):
    import torch

    eng.sync(torch.cuda.current_stream().cuda_stream)


def _same(got, want, label):
    got, want = np.asarray(got).reshape(-1, 8), np.asarray(want).reshape(-1, 8)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (label, "first differing point %d of %d (%d differ)" % (int(bad[0]), len(got), len(bad)))


def _plan(form):
    from b2f import _lib

    p = _lib.fixed_base_plan(1, form)
    return p["window_bits"], p["windows"]


def _base(cv, multiple):
    """The packed point [multiple] G (None: the generator itself)."""
    return mr.pack_points(cv, [mr.gen_mul(cv, multiple)])[0]


def _run(engine, form, scalars, multiple=1, packed=None):
    """The device's points for `scalars` (ints) on the base [multiple] G, and the reference's."""
    cv = mr.curve_of_form(form)
    base = None if (multiple == 1 and packed is None) else (_base(cv, multiple) if packed is None else packed)
    out = engine.fixed_base_mul(_dev(mr.pack_scalars(form, scalars)), base=base, form=form)
    _sync(engine)
    return _host(out), mr.pack_points(cv, fb.expected(form, scalars, multiple))


# ---------------------------------------------------------------------------------------------
# 1. / 2. lengths and forms


@pytest.mark.parametrize("cv", [0, 1])
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(engine, n, cv):
    form = 2 * cv + (n & 1)
    r = mr.ORDER[cv]
    rng = random.Random(3100 + 7 * n + cv)
    scalars = [rng.randrange(r) for _ in range(n)]
    got, want = _run(engine, form, scalars, BASE_MULTIPLE[cv])
    _same(got, want, (n, cv))
    assert got.any(axis=1).all()


@pytest.mark.parametrize("cv", [0, 1])
def test_canonical_and_montgomery_scalars_give_the_same_points(engine, cv):
    r = mr.ORDER[cv]
    rng = random.Random(3200 + cv)
    scalars = [rng.randrange(r) for _ in range(257)]
    scalars[0], scalars[1], scalars[256] = 0, 1, r - 1
    got_c, want = _run(engine, 2 * cv, scalars)
    got_m, _ = _run(engine, 2 * cv + 1, scalars)
    _same(got_c, want, ("canonical", cv))
    _same(got_m, want, ("montgomery", cv))
    assert not got_c[0].any() and got_c[1:].any(axis=1).all()


# ---------------------------------------------------------------------------------------------
# 3. / 4. the recoding


def _steering(cv, c, windows):
    r = mr.ORDER[cv]
    half, top = 1 << (c - 1), windows - 1
    s = [0, 1, r - 1, r - 2, (r - 1) // 2]
    s += [v for v in ((1 << 254) - 1, (1 << 254) + 1) if v < r]
    for d in (half, half - 1, half + 1):  # every digit equal: the carry chains
        s.append(sum(d << (w * c) for w in range(windows)) % r)
    for w in range(windows):
        unit = 1 << (w * c)
        # one non-zero digit: +1 (the scalar 2^(w c)) and the largest entry (the top window's is
        # 2^255 > r, reduced); -1 as r - unit, the point -unit B, and as the digit itself beside a +1
        # in the window above; 2^(w c) - 1
        s += [unit % r, (half * unit) % r, (r - unit) % r, unit - 1]
        if w < top:
            s.append((1 << ((w + 1) * c)) - unit)
    return s


@pytest.mark.parametrize("cv", [0, 1])
def test_scalars_that_steer_the_recoding(engine, cv):
    c, windows = _plan(2 * cv)
    r = mr.ORDER[cv]
    scalars = _steering(cv, c, windows)
    digits = [fb.recode(v, c, windows) for v in scalars]  # none carries out of the top window
    assert all(fb.value(d, c) == v for d, v in zip(digits, scalars))
    flat = {x for d in digits for x in d}
    half = 1 << (c - 1)
    assert {half, 1 - half, -1, 1, 0} <= flat and max(flat) == half and min(flat) == 1 - half
    for form in (2 * cv, 2 * cv + 1):
        for multiple in (1, BASE_MULTIPLE[cv]):
            got, want = _run(engine, form, scalars, multiple)
            _same(got, want, ("steering", form, multiple == 1))


@pytest.mark.parametrize("cv", [0, 1])
def test_partial_sums_that_meet_the_addend(engine, cv):
    c, windows = _plan(2 * cv)
    r = mr.ORDER[cv]
    dbl = fb.doubling_scalar(c, windows, r)
    assert fb.meets(dbl, c, windows, r) == {"double"}
    assert fb.meets(r, c, windows, r) == {"cancel"}  # unreduced: the only scalar that ends in P - P
    rng = random.Random(3300 + cv)
    assert not fb.meets(rng.randrange(r), c, windows, r)
    for multiple in (1, BASE_MULTIPLE[cv]):
        for form in (2 * cv, 2 * cv + 1):
            got, want = _run(engine, form, [dbl, 1, dbl], multiple)
            _same(got, want, ("P + P", form))
        got, _ = _run(engine, 2 * cv, [r, 1, r - 1, r], multiple)  # canonical limbs of r itself
        want = mr.pack_points(cv, [None] + fb.expected(2 * cv, [1, r - 1], multiple) + [None])
        _same(got, want, ("P - P", cv))


# ---------------------------------------------------------------------------------------------
# 5. bases


@pytest.mark.parametrize("cv", [0, 1])
def test_bases(engine, cv):
    form = 2 * cv + 1
    r = mr.ORDER[cv]
    rng = random.Random(3400 + cv)
    scalars = [0, 1, 2, r - 1] + [rng.randrange(r) for _ in range(61)]
    for multiple in (1, rng.randrange(2, r), r - 1):
        got, want = _run(engine, form, scalars, multiple)
        _same(got, want, ("base multiple", multiple))
    # the generator passed explicitly, as a pair and packed, is the default
    dflt = _host(engine.fixed_base_mul(_dev(mr.pack_scalars(form, scalars)), form=form))
    pair = _host(engine.fixed_base_mul(_dev(mr.pack_scalars(form, scalars)), base=mr.GEN[cv], form=form))
    _sync(engine)
    _same(pair, dflt, "the generator as a pair")
    got, _ = _run(engine, form, scalars, packed=np.zeros(8, dtype=np.uint64))
    assert not got.any(), "the identity base gives identities"


@pytest.mark.parametrize("cv", [0, 1])
def test_an_off_curve_base_touches_nothing_else(cv):
    import arena
    import b2f
    import torch

    form, n = 2 * cv + 1, 130
    r = mr.ORDER[cv]
    rng = random.Random(3500 + cv)
    ints = [rng.randrange(r) for _ in range(n)]
    scalars = mr.pack_scalars(form, ints)
    bad =mr.pack_points(cv, [(3, 4)])[0]
    assert not mr.on_curve(cv, (3, 4))
    eng = b2f.Engine(0)
    try:
        s = torch.cuda.current_stream().cuda_stream
        ar = arena.shared()
        d_s = ar.carve(32 * n, 16, dtype=torch.int64, name="scalars")
        d_o = ar.carve(64 * n, 48, dtype=torch.int64, name="out")
        d_s.copy_(_dev(scalars).reshape(-1))
        eng.fixed_base_mul_dev(bad, d_s.data_ptr(), n, form, d_o.data_ptr(), s)
        try:
            eng.sync(s)
        except b2f.B2FError as e:
            assert e.code == ERR_CHECK
        torch.cuda.synchronize()
        assert ar.first_dirty() is None, ar.first_dirty()
        assert np.array_equal(_host(d_s).reshape(-1, 4), scalars), "the scalars changed"
        # the context is fine afterwards
        eng.fixed_base_mul_dev(_base(cv, 1), d_s.data_ptr(), n, form, d_o.data_ptr(), s)
        eng.sync(s)
        _same(_host(d_o), mr.pack_points(cv, fb.expected(form, ints, 1)), "the good call after it")
        assert ar.first_dirty() is None, ar.first_dirty()
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---------------------------------------------------------------------------------------------
# 6. / 7. the table cache


@pytest.mark.parametrize("cv", [0, 1])
def test_table_cache_alternation_and_eviction(cv):
    import b2f
    import torch

    form = 2 * cv + 1
    r = mr.ORDER[cv]
    rng = random.Random(3600 + cv)
    scalars = [rng.randrange(r) for _ in range(65)]
    d_s = _dev(mr.pack_scalars(form, scalars))
    multiples = [rng.randrange(2, r) for _ in range(5)]
    bases = [_base(cv, m) for m in multiples]
    want = [mr.pack_points(cv, fb.expected(form, scalars, m)) for m in multiples]
    eng = b2f.Engine(0)
    try:
        s = torch.cuda.current_stream().cuda_stream
        eng.set_timing(True)
        order = [0, 1, 0] + [0, 1, 2, 3, 4, 0] + [4, 4]
        outs = [eng.fixed_base_mul(d_s, base=bases[i], form=form) for i in order]  # no sync between
        eng.sync(s)
        for i, out in zip(order, outs):
            _same(_host(out), want[i], ("cache", cv, i))
        times = eng.kernel_times()
        assert times["quotient"][1] == len(order)  # one region a call, with or without a build
        assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "quotient")
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---------------------------------------------------------------------------------------------
# 8. / 9. the set-up


@pytest.mark.parametrize("cv", [0, 1])
def test_kzg_setup_is_the_powers_of_tau(engine, cv):
    k, n, form = 10, 1 << 10, 2 * cv + 1
    r = mr.ORDER[cv]
    tau = random.Random(3700 + cv).randrange(2, r)
    g, lag = engine.kzg_setup(k, tau, form=form)
    g_only, none = engine.kzg_setup(k, tau, form=form, lagrange=False)
    _sync(engine)
    powers = [pow(tau, i, r) for i in range(n)]
    _same(_host(g), mr.pack_points(cv, gn.gen_mul_many(cv, powers)), ("g", cv))
    _same(_host(g_only), _host(g), "lagrange=False")
    assert none is None
    want = gn.multiples(cv, powers, k, True)
    sample = [0, 1, 2, 511, 512, 1000, n - 1]
    _same(_host(lag)[sample], mr.pack_points(cv, gn.gen_mul_many(cv, [want[i] for i in sample])), ("g_lagrange", cv))


@pytest.mark.parametrize("cv", [0, 1])
def test_commitment_against_g_is_the_evaluation_at_tau(engine, cv):
    import torch

    k, n, form = 10, 1 << 10, 2 * cv + 1
    r = mr.ORDER[cv]
    rng = random.Random(3800 + cv)
    tau = rng.randrange(2, r)
    cols = [[rng.randrange(r) for _ in range(n)] for _ in range(3)]
    cols[0][0], cols[1][n - 1], cols[2][1] = 0, r - 1, 1
    d_cols = _dev(np.stack([mr.pack_scalars(form, c) for c in cols]))
    g, _ = engine.kzg_setup(k, tau, form=form, lagrange=False)
    commits = engine.msm(d_cols, g, form=form)
    evals = engine.poly_eval(d_cols, [tau], [(c, 0) for c in range(3)], form=form)
    points = engine.fixed_base_mul(evals, form=form)
    _sync(engine)
    assert torch.equal(commits, points)
    ev = [sum(a * pow(tau, i, r) for i, a in enumerate(c)) % r for c in cols]
    _same(_host(points), mr.pack_points(cv, fb.expected(form, ev, 1)), ("[col(tau)] G", cv))


# ---------------------------------------------------------------------------------------------
# 10. a caller's stream


def test_on_a_side_stream_queued_behind_an_msm():
    from test_gpu_side_stream import _cold_then_queued

    cv, form, msm_len, n = 1, 3, 3000, 257
    r = mr.ORDER[cv]
    gm, pts = mr.known_bases(form, msm_len)
    g_packed = mr.pack_points(cv, pts)

    def prepare(eng, run):
        rng = random.Random(3900 + run)
        if run == 0:  # every cache slot allocated, so the queued run's new base refills one in stream order
            import torch

            one = _dev(mr.pack_scalars(form, [1]))
            for m in range(2, 6):
                eng.fixed_base_mul(one, base=_base(cv, m), form=form)
            eng.sync(torch.cuda.current_stream().cuda_stream)
        cols = [[rng.randrange(r) for _ in range(msm_len)] for _ in range(5)]
        scalars = [rng.randrange(r) for _ in range(n)]
        multiple = rng.randrange(2, r)
        return dict(bases=_dev(g_packed), sc=_dev(np.stack([mr.pack_scalars(form, c) for c in cols])),
                    msm=mr.pack_points(cv, [mr.expected_msm(form, c, gm) for c in cols]),
                    s=_dev(mr.pack_scalars(form, scalars)), base=_base(cv, multiple),
                    want=mr.pack_points(cv, fb.expected(form, scalars, multiple)),
                    commit=mr.pack_points(cv, [mr.expected_msm(form, scalars, [v * multiple % r for v in scalars])]))

    def issue(eng, data, mark):
        first = eng.msm(data["sc"], data["bases"], len=msm_len, form=form)
        if mark():
            return None
        pts_ = eng.fixed_base_mul(data["s"], base=data["base"], form=form)  # behind the MSM: table, then multiples
        again = eng.fixed_base_mul(data["s"], base=data["base"], form=form)  # the cached table
        commit = eng.msm(data["s"][None], pts_, form=form)                   # an MSM that reads what it wrote
        return first, pts_, again, commit

    def check(data, outs):
        first, pts_, again, commit = outs
        _same(_host(first), data["msm"], "the MSM in front")
        _same(_host(pts_), data["want"], "the multiples")
        _same(_host(again), data["want"], "the multiples from the cached table")
        _same(_host(commit), data["commit"], "the commitment against them")

    _cold_then_queued("fixbase", prepare, issue, check)


# ---------------------------------------------------------------------------------------------
# 11. the least alignment


@pytest.mark.parametrize("cv", [0, 1])
def test_sixteen_byte_only_pointers_and_guard_bands(engine, cv):
    import arena
    import torch

    form, n = 2 * cv, 193
    r = mr.ORDER[cv]
    rng = random.Random(4000 + cv)
    scalars = [rng.randrange(r) for _ in range(n)]
    packed = mr.pack_scalars(form, scalars)
    ar = arena.shared()
    d_s = ar.carve(32 * n, 16, dtype=torch.int64, name="scalars")
    d_o = ar.carve(64 * n, 112, dtype=torch.int64, name="out")
    assert d_s.data_ptr() % 32 == 16 and d_o.data_ptr() % 32 == 16
    d_s.copy_(_dev(packed).reshape(-1))
    s = torch.cuda.current_stream().cuda_stream
    engine.fixed_base_mul_dev(_base(cv, BASE_MULTIPLE[cv]), d_s.data_ptr(), n, form, d_o.data_ptr(), s)
    engine.sync(s)
    _same(_host(d_o), mr.pack_points(cv, fb.expected(form, scalars, BASE_MULTIPLE[cv])), ("carved", cv))
    assert np.array_equal(_host(d_s).reshape(-1, 4), packed)
    assert ar.first_dirty() is None, ar.first_dirty()


# ---------------------------------------------------------------------------------------------
# 12. refusals


def test_refused_arguments_launch_nothing_and_the_next_call_works():
    import b2f
    import torch

    cv, form, n = 0, 1, 64
    r = mr.ORDER[cv]
    rng = random.Random(4100)
    scalars = [rng.randrange(r) for _ in range(n)]
    packed = mr.pack_scalars(form, scalars)
    want = mr.pack_points(cv, fb.expected(form, scalars, 1))
    base = _base(cv, 1)
    eng = b2f.Engine(0)
    try:
        s = torch.cuda.current_stream().cuda_stream
        d_s = _dev(np.concatenate([packed, packed, packed]))  # room for the overlap cases
        d_o = torch.zeros((2 * n, 8), dtype=torch.int64, device="cuda:0")
        S, O = d_s.data_ptr(), d_o.data_ptr()

        def call(d_scalars=S, len_=n, form=form, d_out=O):
            eng.fixed_base_mul_dev(base, d_scalars, len_, form, d_out, s)

        eng.set_timing(True)
        refused = [dict(d_scalars=0), dict(d_out=0), dict(d_scalars=S + 8), dict(d_out=O + 8), dict(form=4),
                   dict(form=2**31), dict(len_=0), dict(len_=(1 << 28) + 1),
                   dict(d_out=S), dict(d_out=S + 32 * (n - 1)), dict(d_out=S + 32 * n, d_scalars=S + 32 * 2 * n),
                   dict(d_scalars=O + 64 * n - 32)]
        for kw in refused:
            with pytest.raises(b2f.B2FError) as e:
                call(**kw)
            assert e.value.code == ERR_ARG, kw
        assert eng.lib.b2f_fixed_base_mul_dev(eng.ctx, None, S, n, form, O, s) == ERR_ARG  # a null base
        assert eng.lib.b2f_fixed_base_mul_dev(None, None, S, n, form, O, s) == ERR_ARG
        eng.sync(s)
        assert not _host(d_o).any(), "a refused call wrote its output"
        assert np.array_equal(_host(d_s), np.concatenate([packed, packed, packed])), "a refused call wrote its input"
        call()
        eng.sync(s)
        _same(_host(d_o)[:n], want, "the good call after the refusals")
        assert not _host(d_o)[n:].any(), "rows past len were written"
        times = eng.kernel_times()
        assert times["quotient"][1] == 1 and times["quotient"][0] > 0  # one region, the good call's
        assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "quotient")
        # adjacent buffers do not overlap
        d_t = torch.zeros((3 * n, 4), dtype=torch.int64, device="cuda:0")
        d_t[:n] = d_s[:n]
        call(d_scalars=d_t.data_ptr(), d_out=d_t.data_ptr() + 32 * n)
        eng.sync(s)
        _same(_host(d_t)[n:].reshape(-1, 8), want, "output right behind the scalars")
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_host_tensors_are_refused_by_the_tensor_call(engine):
    import b2f
    import torch

    host = torch.from_numpy(mr.pack_scalars(1, [1, 2, 3]).view(np.int64))
    dev = host.to("cuda:0")
    for kw in (dict(scalars=host), dict(scalars=dev, out=torch.empty((3, 8), dtype=torch.int64)),
               dict(scalars=dev.reshape(-1)), dict(scalars=dev, out=torch.empty((2, 8), dtype=torch.int64, device="cuda:0"))):
        with pytest.raises(b2f.B2FError) as e:
            engine.fixed_base_mul(kw["scalars"], form=1, out=kw.get("out"))
        assert e.value.code == ERR_ARG, kw.keys()
    _sync(engine)
