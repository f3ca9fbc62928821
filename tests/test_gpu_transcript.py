"""b2f_transcript_*_dev (csrc/b2f_transcript.hip) against the pure-Python restatement of
tests/transcript_ref.py (pinned to hashlib by tests/test_transcript_ref.py), word for word.

  1  mixed sequences of points, scalars and squeezes whose length at a squeeze's finalisation is 127,
     128 and 129 bytes modulo 128: after every step the 32 state words and every challenge, all four
     forms;
  2  n in {1, 2, 255, 256, 257, 1025} elements absorbed in one call against the same elements one at
     a time (the chunk boundary of the converting lanes), and against the restatement;
  3  points and scalars with coordinates 0, 1 and p - 1;
  4  the identity point: B2F_ERR_FIELD at sync, the state as defined, the next call good;
  5  the wide reduction (a + b 2^256 mod r) through the diagnostics op on the edges a hash output
     never lands on, against Python integers;
  6  every refused argument: its code, no timing region, a good call afterwards;
  7  the calls on a non-blocking side stream behind in-flight work.

Needs an MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import msm_ref as mr
import transcript_ref as tr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FIELD = 1, 7
FORMS = [0, 1, 2, 3]


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _sync(eng):
    import torch

    eng.sync(torch.cuda.current_stream().cuda_stream)


def _words(t):
    return np.array(t.words(), dtype=np.uint64)


def _limbs(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64).copy()


class Pair:
    """A device transcript and its restatement, moved in step."""

    def __init__(self, eng, form):
        self.eng, self.form, self.cv = eng, form, mr.curve_of_form(form)
        self.ref = tr.Transcript(self.cv)
        self.state = eng.transcript_init()

    def points(self, pts):
        self.eng.transcript_absorb_points(self.state, _dev(mr.pack_points(self.cv, pts)), form=self.form)
        for pt in pts:
            self.ref.common_point(pt)

    def scalars(self, vals):
        self.eng.transcript_absorb_scalars(self.state, _dev(mr.pack_scalars(self.form, vals)), form=self.form)
        for v in vals:
            self.ref.common_scalar(v)

    def squeeze(self):
        got = self.eng.transcript_squeeze(self.state, form=self.form)
        want = self.ref.squeeze()
        _sync(self.eng)
        assert np.array_equal(_host(got), _limbs(want)), ("challenge", self.form)
        return want

    def check(self, tag):
        _sync(self.eng)
        assert np.array_equal(_host(self.state), _words(self.ref)), ("state", self.form, tag)


@pytest.mark.parametrize("form", FORMS)
def test_sequences_at_the_block_edges(engine, form):
    cv = mr.curve_of_form(form)
    r = mr.ORDER[cv]
    rng = random.Random(60 + form)
    pt = mr.gen_mul(cv, rng.randrange(1, r))
    s = rng.randrange(r)
    t = Pair(engine, form)
    t.check("init")
    lengths = []
    # one point, one scalar and thirty squeezes is exactly 128 bytes; the thirty-first is 129
    steps = [("point", pt), ("scalar", s)] + [("squeeze", None)] * 31
    # and two blocks later, points and scalars between the squeezes: 129 + 33 + 65 + 1 + 33 + 33 + 65 = 359
    steps += [("scalar", s), ("point", pt), ("squeeze", None), ("scalar", 0), ("scalar", r - 1), ("point", pt)]
    steps += [("squeeze", None)] * 26
    for i, (kind, val) in enumerate(steps):
        if kind == "point":
            t.points([val])
        elif kind == "scalar":
            t.scalars([val])
        else:
            t.squeeze()
            lengths.append(t.ref.hash.t + t.ref.hash.count)
        t.check((i, kind))
    assert lengths[28:31] == [127, 128, 129] and lengths[-3:] == [383, 384, 385]


_elements = {}


def _many(cv, n):
    """n points (the pool's, cycled) and n scalars of the curve, built once."""
    if cv not in _elements:
        rng = random.Random(70 + cv)
        _elements[cv] = (mr.known_bases(2 * cv, 1025)[1], [rng.randrange(mr.ORDER[cv]) for _ in range(1025)])
    pts, vals = _elements[cv]
    return pts[:n], vals[:n]


@pytest.mark.parametrize("kind", ["points", "scalars"])
@pytest.mark.parametrize("form", FORMS)
def test_one_call_against_one_at_a_time(engine, form, kind):
    cv = mr.curve_of_form(form)
    for n in (1, 2, 255, 256, 257, 1025):
        pts, vals = _many(cv, n)
        whole = Pair(engine, form)
        whole.scalars([5])  # off the block's start: the chunks do not line up with the buffer
        single = engine.transcript_init()
        engine.transcript_absorb_scalars(single, _dev(mr.pack_scalars(form, [5])), form=form)
        if kind == "points":
            whole.points(pts)
            d = _dev(mr.pack_points(cv, pts))
            for i in range(n):
                engine.transcript_absorb_points(single, d[i:i + 1], form=form)
        else:
            whole.scalars(vals)
            d = _dev(mr.pack_scalars(form, vals))
            for i in range(n):
                engine.transcript_absorb_scalars(single, d[i:i + 1], form=form)
        whole.check((kind, n))
        assert np.array_equal(_host(single), _host(whole.state)), (form, kind, n)
        whole.squeeze()


@pytest.mark.parametrize("form", FORMS)
def test_edge_coordinates(engine, form):
    cv = mr.curve_of_form(form)
    q, r = mr.Q[cv], mr.ORDER[cv]
    t = Pair(engine, form)
    # the coordinates are not checked to be on the curve; (0, 0) is the identity and has its own test
    t.points([(0, 1), (1, 0), (1, 1), (q - 1, q - 1), (0, q - 1), (q - 1, 0), (1, q - 1)])
    t.check("points")
    t.scalars([0, 1, r - 1, 1, 0])
    t.check("scalars")
    t.squeeze()
    t.check("squeeze")


@pytest.mark.parametrize("form", FORMS)
def test_identity_point(engine, form):
    from b2f import B2FError

    cv = mr.curve_of_form(form)
    pt = mr.gen_mul(cv, 12345)
    t = Pair(engine, form)
    t.points([pt, None, pt])
    with pytest.raises(B2FError) as e:
        _sync(engine)
    assert e.value.code == ERR_FIELD
    # the byte 1 and 64 zero bytes went in: the state is the restatement's
    assert t.ref.hash.t + t.ref.hash.count == 3 * 65
    t.check("after the identity")
    t.points([pt])
    t.squeeze()
    t.check("the next call")


@pytest.mark.parametrize("field", [0, 1])
def test_wide_reduction(diag_engine, field):
    r = mr.ORDER[field]
    rng = random.Random(90 + field)
    top = (1 << 256) - 1
    wide = [0, r - 1, r, top, (r - 1) << 256, (1 << 512) - 1,
            r << 256, (r << 256) + r - 1, (r << 256) + r, (top << 256) + r - 1, 1 << 256, r + 1, 2 * r - 1, 2 * r]
    wide += [rng.randrange(1 << 512) for _ in range(64)]
    a = np.stack([_limbs(x & top) for x in wide])
    b = np.stack([_limbs(x >> 256) for x in wide])
    got = diag_engine.debug_reduce_wide(a, b, field)
    want = np.stack([_limbs(x % r) for x in wide])
    bad = [hex(wide[i]) for i in range(len(wide)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad


def test_the_product_library_has_no_debug_name():
    import b2f

    assert not hasattr(b2f.load(), "b2f_debug_field_op")


def test_refused_arguments(engine):
    import torch

    from b2f import B2FError

    form, cv = 1, 0
    pts, vals = _many(cv, 4)
    d_pts, d_vals = _dev(mr.pack_points(cv, pts)), _dev(mr.pack_scalars(form, vals))
    state = torch.zeros(32 + 8, dtype=torch.int64, device="cuda:0")
    chal = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    S, PT, SC, CH = state.data_ptr(), d_pts.data_ptr(), d_vals.data_ptr(), chal.data_ptr()
    ref = tr.Transcript(cv)
    for pt in pts:
        ref.common_point(pt)
    for v in vals:
        ref.common_scalar(v)
    want = ref.squeeze()

    def good():
        engine.transcript_init_dev(S, s)
        engine.transcript_absorb_points_dev(S, PT, 4, form, s)
        engine.transcript_absorb_scalars_dev(S, SC, 4, form, s)
        engine.transcript_squeeze_dev(S, form, CH, s)
        engine.sync(s)
        assert np.array_equal(_host(chal), _limbs(want))
        assert np.array_equal(_host(state)[:32], _words(ref))

    good()
    big = (1 << 20) + 1
    refused = [(engine.transcript_init_dev, (0,)), (engine.transcript_init_dev, (S + 8,))]
    for fn, data in ((engine.transcript_absorb_points_dev, PT), (engine.transcript_absorb_scalars_dev, SC)):
        refused += [(fn, (0, data, 4, form)), (fn, (S, 0, 4, form)), (fn, (S + 8, data, 4, form)),
                    (fn, (S, data + 8, 2, form)), (fn, (S, data, 4, 4)), (fn, (S, data, 0, form)),
                    (fn, (S, data, big, form)),
                    (fn, (S, S + 128, 1, form)), (fn, (S, S + 256 - 32, 2, form)),  # the data in the state
                    (fn, (data + 64, data, 4, form))]                               # the state in the data
    refused += [(engine.transcript_squeeze_dev, (0, form, CH)), (engine.transcript_squeeze_dev, (S, form, 0)),
                (engine.transcript_squeeze_dev, (S + 8, form, CH)), (engine.transcript_squeeze_dev, (S, form, CH + 8)),
                (engine.transcript_squeeze_dev, (S, 4, CH)), (engine.transcript_squeeze_dev, (S, form, S + 64)),
                (engine.transcript_squeeze_dev, (S, form, S + 224))]
    for fn, args in refused:
        engine.set_timing(True)
        with pytest.raises(B2FError) as e:
            fn(*args, s)
        assert e.value.code == ERR_ARG, (fn.__name__, args)
        times = engine.kernel_times()
        engine.set_timing(False)
        assert all(v[1] == 0 for v in times.values()), (fn.__name__, args)
    good()
    # the words past the state were never written
    assert not _host(state)[32:].any()
    # each good call is one region of the quotient kind
    engine.set_timing(True)
    engine.transcript_init_dev(S, s)
    engine.transcript_absorb_points_dev(S, PT, 4, form, s)
    engine.transcript_absorb_scalars_dev(S, SC, 4, form, s)
    engine.transcript_squeeze_dev(S, form, CH, s)
    times = engine.kernel_times()
    engine.set_timing(False)
    assert times["quotient"][1] == 4 and times["quotient"][0] > 0
    assert all(v[1] == 0 for k, v in times.items() if k != "quotient")


def test_on_a_side_stream_behind_in_flight_work():
    """The four calls, a hundred of them, on a non-blocking stream behind a filler of matmuls, with
    no host synchronisation until the end; the filler is still pending when the first call returns."""
    import b2f
    import torch

    form, cv = 3, 1
    pts, vals = _many(cv, 300)
    ref = tr.Transcript(cv)
    want = []
    for i in range(25):
        for pt in pts[12 * i:12 * i + 12]:
            ref.common_point(pt)
        for v in vals[7 * i:7 * i + 7]:
            ref.common_scalar(v)
        want.append(ref.squeeze())
    side = torch.cuda.Stream()
    eng = b2f.Engine(0)
    try:
        with torch.cuda.stream(side):
            d_pts, d_vals = _dev(mr.pack_points(cv, pts)), _dev(mr.pack_scalars(form, vals))
            a = torch.rand((2048, 2048), device="cuda:0")
            out = torch.empty_like(a)
            torch.matmul(a, a, out=out)
            warm = eng.transcript_init(stream=side.cuda_stream)  # the context's first call
            eng.sync(side.cuda_stream)
            for _ in range(100):
                torch.matmul(a, a, out=out)
            filler_done = torch.cuda.Event()
            filler_done.record(side)
            state = eng.transcript_init(stream=side.cuda_stream)
            pending = not filler_done.query()
            chal = torch.zeros((25, 4), dtype=torch.int64, device="cuda:0")
            for i in range(25):
                eng.transcript_absorb_points(state, d_pts[12 * i:12 * i + 12], form=form, stream=side.cuda_stream)
                eng.transcript_absorb_scalars(state, d_vals[7 * i:7 * i + 7], form=form, stream=side.cuda_stream)
                eng.transcript_squeeze(state, form=form, out=chal[i], stream=side.cuda_stream)
            eng.sync(side.cuda_stream)
            assert pending, "the first call returned after the filler had finished: nothing was queued"
            assert np.array_equal(_host(chal), np.stack([_limbs(w) for w in want]))
            assert np.array_equal(_host(state), _words(ref))
            del warm
    finally:
        torch.cuda.synchronize()
        eng.close()
