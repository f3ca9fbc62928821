"""b2f_group_ntt_dev (csrc/b2f_group_ntt.hip: the group NTT, g -> g_lagrange) on the MI355X, bit
for bit against the big-integer reference tests/group_ntt_ref.py. The inputs are known multiples of
the generator (msm_ref.known_bases), so the expected transform is a field NTT of the multiples and
one fixed-base multiplication per output.

  1  sizes: k = 1, 2, 3 (one butterfly, the first real twiddle, the first multi-stage case), 6 and
     7 (stage 1 has 64 blocks or more, but it has no twiddle: every twiddle stage is still the
     mixed-twiddle kernel), 8 (the change-over: stage 2 is the first twiddle-uniform launch, with
     exactly 64 blocks, so a wave is exactly one twiddle group), 10 (several workgroups, three
     uniform stages), 12 (the largest); both curves, both directions;
  2  all inputs equal at k = 7: every a - t meets opposite points and a + t a doubling;
  3  one non-identity input among identities, and all identities, at k = 6;
  4  forward(inverse(g)) == g at k = 9, in place and out of place (the input untouched);
  5  the defining property on the device at k = 10: the commitment of a Lagrange column against
     inverse(g) is the commitment of its coefficients against g, for a random column (Engine.msm)
     and for a trace's advice columns (DeviceBatch.commit_advice);
  6  refusals: every B2F_ERR_ARG case launches nothing and the next good call is right; a
     generator of half the order raises B2F_ERR_FIELD at sync and the next call works;
  7  the call on a caller's non-blocking stream, queued behind an in-flight MSM.

Needs an MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import group_ntt_ref as gn
import msm_ref as mr
import ntt_ref as nr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FIELD = 1, 7
FWD, INV = 0, 1
KS = [1, 2, 3, 6, 7, 8, 10, 12]
_inputs = {}


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


def _known(cv, k):
    """(multiples, packed points) of 2^k distinct known multiples of G, built once: the pool, and
    past its 1,024 entries the incremental family (the pool cycled would be a periodic input,
    whose transform is the identity at three outputs of four)."""
    if (cv, k) not in _inputs:
        n = 1 << k
        bs, pts = mr.known_bases(2 * cv, min(n, mr.POOL_SIZE))
        if n > mr.POOL_SIZE:
            fb, fp = mr.known_bases(2 * cv, n - mr.POOL_SIZE, incremental=True)
            bs, pts = bs + fb, pts + fp
        _inputs[(cv, k)] = (bs, mr.pack_points(cv, pts))
    return _inputs[(cv, k)]


def _want(cv, b, k, inverse):
    return mr.pack_points(cv, gn.transform_known(cv, b, k, inverse))


# ---------------------------------------------------------------------------------------------
# 1. sizes


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("cv", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_sizes_against_the_known_multiples(engine, k, cv, inverse):
    import torch

    b, packed = _known(cv, k)
    form = 2 * cv + (k & 1)  # the form only selects the curve: both forms of each
    d_in = _dev(packed)
    out = engine.group_ntt(d_in, k, inverse=inverse, form=form)
    _sync(engine)
    assert torch.equal(d_in, _dev(packed)), "the call changed its input"
    _same(_host(out), _want(cv, b, k, inverse), (k, cv, inverse))


# ---------------------------------------------------------------------------------------------
# 2. / 3. structured inputs


@pytest.mark.parametrize("cv", [0, 1])
def test_all_inputs_equal(engine, cv):
    k, n, form = 7, 1 << 7, 2 * cv + 1
    m = 0x1234567 + cv
    p = mr.gen_mul(cv, m)
    d_in = _dev(mr.pack_points(cv, [p] * n))
    inv = engine.g_to_lagrange(d_in, k, form=form)
    fwd = engine.group_ntt(d_in, k, form=form)
    _sync(engine)
    _same(_host(inv), mr.pack_points(cv, [p] + [None] * (n - 1)), ("inverse of a constant", cv))
    _same(_host(fwd), mr.pack_points(cv, [mr.gen_mul(cv, m * n)] + [None] * (n - 1)), ("forward of a constant", cv))


@pytest.mark.parametrize("cv", [0, 1])
def test_one_point_among_identities_and_all_identities(engine, cv):
    k, n, form = 6, 1 << 6, 2 * cv + 1
    for j0 in (0, 1, 37, n - 1):
        b = [0] * n
        b[j0] = 0xabcdef0123456789 + j0
        d_in = _dev(mr.pack_points(cv, [mr.gen_mul(cv, v) if v else None for v in b]))
        for inverse in (False, True):
            out = engine.group_ntt(d_in, k, inverse=inverse, form=form)
            _sync(engine)
            _same(_host(out), _want(cv, b, k, inverse), ("one point at", j0, cv, inverse))
    zeros = np.zeros((n, 8), dtype=np.uint64)
    for inverse in (False, True):
        out = engine.group_ntt(_dev(zeros), k, inverse=inverse, form=form)
        _sync(engine)
        _same(_host(out), zeros, ("all identities", cv, inverse))


# ---------------------------------------------------------------------------------------------
# 4. round trip


@pytest.mark.parametrize("cv", [0, 1])
def test_round_trip_in_place_and_out_of_place(engine, cv):
    import torch

    k, form = 9, 2 * cv + 1
    b, packed = _known(cv, k)
    want_inv = _want(cv, b, k, True)
    # out of place
    d_g = _dev(packed)
    lag = engine.g_to_lagrange(d_g, k, form=form)
    back = engine.group_ntt(lag, k, form=form)
    _sync(engine)
    assert torch.equal(d_g, _dev(packed)), "out of place: the input changed"
    _same(_host(lag), want_inv, ("out of place inverse", cv))
    _same(_host(back), packed, ("out of place round trip", cv))
    # in place, with a row past 2^k that must stay
    buf = _dev(np.concatenate([packed, np.full((1, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)]))
    assert engine.g_to_lagrange(buf, k, form=form, out=buf) is buf
    _sync(engine)
    _same(_host(buf)[:-1], want_inv, ("in place inverse", cv))
    engine.group_ntt(buf, k, form=form, out=buf)
    _sync(engine)
    _same(_host(buf)[:-1], packed, ("in place round trip", cv))
    assert (_host(buf)[-1] == np.uint64(0x5A5A5A5A5A5A5A5A)).all(), "the row past 2^k was written"


# ---------------------------------------------------------------------------------------------
# 5. the defining property


@pytest.mark.parametrize("cv", [0, 1])
def test_lagrange_commitment_equals_coefficient_commitment(engine, cv):
    import torch

    k, n, form = 10, 1 << 10, 2 * cv + 1
    r = mr.ORDER[cv]
    b, packed = _known(cv, k)
    rng = np.random.default_rng(2100 + cv)
    cols = [nr.random_elements(rng, n, r) for _ in range(2)]
    cols[0][0], cols[0][n - 1], cols[1][5] = 0, r - 1, 1
    d_cols = _dev(np.stack([nr.pack(c, form) for c in cols]))
    d_g = _dev(packed)
    d_lag = engine.g_to_lagrange(d_g, k, form=form)
    by_lagrange = engine.msm(d_cols, d_lag, form=form)
    coeff = engine.ntt_columns(d_cols, k, inverse=True, form=form)
    by_coeff = engine.msm(coeff, d_g, form=form)
    _sync(engine)
    assert torch.equal(by_lagrange, by_coeff)
    # and the big integers: the coefficients against the multiples of g
    w = gn.omega(cv, k)
    want = [mr.expected_msm(form, nr.inverse(c, k, w, 1, r), b) for c in cols]
    _same(_host(by_lagrange), mr.pack_points(cv, want), ("commitments", cv))
    assert all(p is not None for p in want)


@pytest.mark.parametrize("cv", [0, 1])
def test_commit_advice_against_the_produced_g_lagrange(engine, cv):
    import torch

    import b2f
    from b2f import synth

    k, n, form, tail_rows = 10, 1 << 10, 2 * cv + 1, 6
    r = mr.ORDER[cv]
    x = synth.batch(2, rounds_mix=[0, 1], seed=78)
    x["rounds"][:] = [1, 0]
    batch = b2f.DeviceBatch(x, device="cuda:0")
    batch.fill_evaluate(engine)
    used = int(batch.offsets_host[-1])
    usable = n - tail_rows
    assert 600 < used <= usable
    rng = random.Random(2200 + cv)
    tail = [[rng.randrange(r) for _ in range(tail_rows)] for _ in range(10)]
    d_tail = _dev(np.stack([mr.pack_scalars(form, t) for t in tail]))
    d_g = _dev(_known(cv, k)[1])
    d_lag = engine.g_to_lagrange(d_g, k, form=form)
    got = batch.commit_advice(engine, 0, usable, d_lag, tail=d_tail, form=form)
    # the exported columns (Lagrange form, blinding rows last), their coefficients, against g
    block = torch.zeros((10, n, 4), dtype=torch.int64, device="cuda:0")
    batch.export_fp(engine, 0, used, form=form, out=block)
    block[:, usable:] = d_tail
    coeff = engine.ntt_columns(block, k, inverse=True, form=form)
    want = engine.msm(coeff, d_g, form=form)
    _sync(engine)
    assert torch.equal(got, want)
    assert len(set(map(tuple, _host(got).tolist()))) == 10 and _host(got).any(axis=1).all()


# ---------------------------------------------------------------------------------------------
# 6. refusals


def test_refused_arguments_launch_nothing_and_the_next_call_works():
    import b2f
    import torch

    cv, k, form = 0, 5, 1
    n = 1 << k
    b, packed = _known(cv, 6)
    b, packed = b[:n], packed[:n]
    want = _want(cv, b, k, True)
    eng = b2f.Engine(0)
    try:
        s = torch.cuda.current_stream().cuda_stream
        d_in = _dev(np.concatenate([packed, packed]))  # room for the overlap cases
        d_out = torch.zeros((2 * n, 8), dtype=torch.int64, device="cuda:0")
        I, O, w = d_in.data_ptr(), d_out.data_ptr(), gn.omega(cv, k)
        r = mr.ORDER[cv]

        def call(d_in=I, k=k, omega=w, direction=INV, form=form, d_out=O):
            eng.group_ntt_dev(d_in, k, omega, direction, form, d_out, s)

        eng.set_timing(True)
        refused = [dict(d_in=0), dict(d_out=0), dict(d_in=I + 8), dict(d_out=O + 8), dict(k=0), dict(k=29),
                   dict(direction=2), dict(form=4), dict(omega=r), dict(omega=2**256 - 1),
                   dict(omega=mr.ORDER[1], form=3),
                   dict(d_out=I + 64), dict(d_out=I + 64 * (n - 1)), dict(d_in=I + 64, d_out=I)]
        for kw in refused:
            with pytest.raises(b2f.B2FError) as e:
                call(**kw)
            assert e.value.code == ERR_ARG, kw
        assert eng.lib.b2f_group_ntt_dev(eng.ctx, I, k, None, INV, form, O, s) == ERR_ARG  # a null omega
        eng.sync(s)
        assert not _host(d_out).any(), "a refused call wrote its output"
        _same(_host(d_in), np.concatenate([packed, packed]), "a refused call wrote its input")
        call()
        eng.sync(s)
        _same(_host(d_out)[:n], want, "the good call after the refusals")
        times = eng.kernel_times()
        assert times["quotient"][1] == 1 and times["quotient"][0] > 0  # one region, the good call's
        assert all(cnt == 0 for name, (_, cnt) in times.items() if name != "quotient")
        # adjacent buffers do not overlap
        call(d_out=I + 64 * n)
        eng.sync(s)
        _same(_host(d_in)[n:], want, "output right behind the input")
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_host_tensors_are_refused_by_the_tensor_call(engine):
    import b2f
    import torch

    k = 3
    host = torch.from_numpy(_known(0, k)[1].view(np.int64))
    dev = host.to("cuda:0")
    for kw in (dict(points=host), dict(points=dev, out=torch.empty_like(host)), dict(points=host, out=dev.clone())):
        with pytest.raises(b2f.B2FError) as e:
            engine.group_ntt(kw["points"], k, form=1, out=kw.get("out"))
        assert e.value.code == ERR_ARG, kw.keys()
    _sync(engine)


@pytest.mark.parametrize("cv", [0, 1])
def test_a_generator_of_half_the_order_raises_at_sync(cv):
    import b2f
    import torch

    k, form = 6, 2 * cv + 1
    b, packed = _known(cv, k)
    eng = b2f.Engine(0)
    try:
        s = torch.cuda.current_stream().cuda_stream
        d_in = _dev(packed)
        out = torch.empty_like(d_in)
        for direction in (FWD, INV):
            for bad in (gn.omega(cv, k - 1), 1, 0):
                eng.group_ntt_dev(d_in.data_ptr(), k, bad, direction, form, out.data_ptr(), s)
                with pytest.raises(b2f.B2FError) as e:
                    eng.sync(s)
                assert e.value.code == ERR_FIELD, (direction, bad)
            eng.group_ntt_dev(d_in.data_ptr(), k, gn.omega(cv, k), direction, form, out.data_ptr(), s)
            eng.sync(s)  # cleared, and the call is right
            _same(_host(out), _want(cv, b, k, direction == INV), ("after the wrong root", cv, direction))
    finally:
        torch.cuda.synchronize()
        eng.close()


# ---------------------------------------------------------------------------------------------
# 7. a caller's stream


def test_on_a_side_stream_queued_behind_an_msm():
    from test_gpu_side_stream import _cold_then_queued

    cv, k, form, msm_len = 0, 7, 1, 3000
    n = 1 << k
    r = mr.ORDER[cv]
    gm, pts = mr.known_bases(form, msm_len)
    g_packed = mr.pack_points(cv, pts)

    def prepare(eng, run):
        rng = random.Random(2300 + run)
        cols = [[rng.randrange(r) for _ in range(msm_len)] for _ in range(5)]
        col = [rng.randrange(r) for _ in range(n)]
        # this run's points: a rotation of the pool, so the two runs transform different inputs
        b = gm[run * n:(run + 1) * n]
        w = gn.omega(cv, k)
        return dict(bases=_dev(g_packed), sc=_dev(np.stack([mr.pack_scalars(form, c) for c in cols])),
                    msm=mr.pack_points(cv, [mr.expected_msm(form, c, gm) for c in cols]),
                    g=_dev(g_packed[run * n:(run + 1) * n]), lag=_want(cv, b, k, True),
                    col=_dev(mr.pack_scalars(form, col)[None]),
                    commit=mr.pack_points(cv, [mr.expected_msm(form, nr.inverse(col, k, w, 1, r), b)]))

    def issue(eng, data, mark):
        first = eng.msm(data["sc"], data["bases"], len=msm_len, form=form)
        if mark():
            return None
        lag = eng.g_to_lagrange(data["g"], k, form=form)   # behind the MSM, whose scratch it does not share
        commit = eng.msm(data["col"], lag, form=form)      # and an MSM that reads what it wrote
        back = eng.group_ntt(lag, k, form=form, out=lag.clone())
        return first, lag, commit, back

    def check(data, outs):
        first, lag, commit, back = outs
        _same(_host(first), data["msm"], "the MSM in front")
        _same(_host(lag), data["lag"], "g_lagrange")
        _same(_host(commit), data["commit"], "the commitment against it")
        _same(_host(back), _host(data["g"]), "forward again")

    _cold_then_queued("groupntt", prepare, issue, check)
