"""b2f_ipa_open_dev (csrc/b2f_ipa.hip, b2f_fixed_base.hip, b2f_transcript.h) against the restatement of
tests/transcript_ref.py, bit for bit, on both curves. The generators are msm_ref.known_bases and U, W
known multiples of the curve's generator, so every expected point is one gen_mul.

  1  whole openings, k = 1..8, all four forms: the transcript pre-loaded with a few points and
     scalars, z squeezed on the device; every L_j, R_j, u_j, c, f, the final state words and the
     first element of the folded p, b, G; poisoned guard rows around every output untouched;
  2  agreement with the existing calls: the three-call loop with the host Caller, driven with the
     u_j the device squeezed, gives the same L_j, R_j, c and f;
  3  one opening at k = 12, forms 1 and 3: rounds on the long Pippenger path;
  4  two openings back to back on one context with different U and W (the table cache takes new
     bases), an msm call between them (the shared scratch);
  5  the tensor-level wrapper;
  6  every refused argument: its code, no timing region, a good call afterwards.

Needs an MI355X (`-m gpu`)."""
import random

import numpy as np
import pytest

import ipa_ref as ir
import msm_ref as mr
import transcript_ref as tr

pytestmark = pytest.mark.gpu

ERR_ARG = 1
POISON = np.uint64(0xfefefefefefefefe)
GUARD = 4  # rows of poison on either side of an output


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _limbs(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64).copy()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


_cases = {}


def _case(form, k, variant=0):
    """Seeded inputs of an opening and its restatement, shared by the tests that run it (per curve:
    the scalars are integers, the form only packs them)."""
    cv = mr.curve_of_form(form)
    key = (cv, k, variant)
    if key not in _cases:
        r = mr.ORDER[cv]
        seed = 5000 + 100 * k + 10 * variant + cv
        rng = random.Random(seed)
        n = 1 << k
        gm, pts = mr.known_bases(form, n)
        c = dict(cv=cv, k=k, n=n, gm=gm, pts=pts, seed=seed)
        c["p"] = [rng.randrange(r) for _ in range(n)]
        c["x"] = rng.randrange(1, r)
        c["um"], c["wm"] = rng.randrange(1, r), rng.randrange(1, r)
        c["f0"] = rng.randrange(r)
        c["pre_pts"] = [mr.gen_mul(cv, rng.randrange(1, r)) for _ in range(3)]
        c["pre_vals"] = [rng.randrange(r) for _ in range(2)]
        # the blinding scalars in the order ipa_ref.Caller(seed) draws them
        draw = random.Random(seed)
        c["rand"] = [draw.randrange(r) for _ in range(2 * k)]
        c["U"], c["W"] = mr.gen_mul(cv, c["um"]), mr.gen_mul(cv, c["wm"])
        t = tr.Transcript(cv)
        for pt in c["pre_pts"]:
            t.common_point(pt)
        for v in c["pre_vals"]:
            t.common_scalar(v)
        c["z"] = t.squeeze()
        c["want"] = tr.opening_known(cv, c["p"], ir.powers(cv, c["x"], n), gm, c["um"], c["wm"], c["z"], c["rand"],
                                     t, c["f0"])
        c["state"] = np.array(t.words(), dtype=np.uint64)
        _cases[key] = c
    return _cases[key]


def _guarded(rows, width):
    import torch

    t = torch.from_numpy(np.full((rows + 2 * GUARD, width), POISON, dtype=np.uint64).view(np.int64)).to("cuda:0")
    return t, t[GUARD:GUARD + rows]


def _run(eng, form, c, check=True):
    """The opening on the device through the pointer-level call, outputs between poisoned guard rows.
    Returns (lr [k, 16], u [k, 4], cf [2, 4], state [32], d_p, d_b, d_g) as host arrays / tensors."""
    cv, k, n = c["cv"], c["k"], c["n"]
    s = _stream()
    d_p, d_g = _dev(mr.pack_scalars(form, c["p"])), _dev(mr.pack_points(cv, c["pts"]))
    d_rand = _dev(mr.pack_scalars(form, c["rand"]))
    state = eng.transcript_init()
    eng.transcript_absorb_points(state, _dev(mr.pack_points(cv, c["pre_pts"])), form=form)
    eng.transcript_absorb_scalars(state, _dev(mr.pack_scalars(form, c["pre_vals"])), form=form)
    d_z = eng.transcript_squeeze(state, form=form)
    d_b = eng.ipa_powers(c["x"], n, form=form)
    lr_all, lr = _guarded(k, 16)
    u_all, u = _guarded(k, 4)
    cf_all, cf = _guarded(2, 4)
    cf[1].copy_(_dev(mr.pack_scalars(form, [c["f0"]]))[0])
    U, W = mr.pack_points(cv, [c["U"], c["W"]])
    eng.ipa_open_dev(d_p.data_ptr(), d_b.data_ptr(), d_g.data_ptr(), n, U, W, d_z.data_ptr(), d_rand.data_ptr(),
                     state.data_ptr(), form, lr.data_ptr(), u.data_ptr(), cf.data_ptr(), s)
    eng.sync(s)
    got = (_host(lr), _host(u), _host(cf), _host(state), d_p, d_b, d_g)
    for name, whole, rows in (("lr", lr_all, k), ("u", u_all, k), ("cf", cf_all, 2)):
        h = _host(whole)
        assert (h[:GUARD] == POISON).all() and (h[GUARD + rows:] == POISON).all(), ("guard rows", name, form, k)
    assert np.array_equal(_host(d_z), _limbs(c["z"])), ("z", form, k)
    if check:
        _check(form, c, got)
    return got


def _check(form, c, got):
    cv, k, want = c["cv"], c["k"], c["want"]
    lr, u, cf, state, d_p, d_b, d_g = got
    tag = (form, k)
    for j in range(k):
        assert np.array_equal(lr[j].reshape(2, 8), mr.pack_points(cv, list(want["lr"][j]))), ("L, R", tag, j)
        assert np.array_equal(u[j], _limbs(want["u"][j])), ("u", tag, j)
    assert np.array_equal(cf, mr.pack_scalars(form, [want["c"], want["f"]])), ("c, f", tag)
    assert np.array_equal(state, c["state"]), ("state", tag)
    assert np.array_equal(_host(d_p)[0], mr.pack_scalars(form, want["p"])[0]), ("p", tag)
    assert np.array_equal(_host(d_b)[0], mr.pack_scalars(form, want["b"])[0]), ("b", tag)
    assert np.array_equal(_host(d_g)[0], mr.pack_points(cv, ir.points_of(cv, want["g"]))[0]), ("G", tag)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_whole_openings(engine, form):
    for k in range(1, 9):
        _run(engine, form, _case(form, k))


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_agreement_with_the_three_calls(engine, form):
    """The host-driven loop of b2f_ipa_round_dev / b2f_ipa_fold_dev with ipa_ref.Caller doing the
    U / W terms by plain point arithmetic, fed the challenges the one call squeezed."""
    cv = mr.curve_of_form(form)
    for k in (1, 3, 8):
        c = _case(form, k)
        lr, u, cf, _, _, _, _ = _run(engine, form, c)
        us = [int.from_bytes(u[j].tobytes(), "little") for j in range(k)]
        caller = ir.Caller(cv, c["U"], c["W"], c["z"], c["f0"], c["seed"])
        d_p, d_g = _dev(mr.pack_scalars(form, c["p"])), _dev(mr.pack_points(cv, c["pts"]))
        d_b = engine.ipa_powers(c["x"], c["n"], form=form)
        ln = c["n"]
        for j in range(k):
            raw, vals = engine.ipa_round(d_p, d_b, d_g, len=ln, form=form)
            engine.sync(_stream())
            L, R = mr.unpack_points(cv, _host(raw))
            r = mr.ORDER[cv]
            vl, vr = [int.from_bytes(v.tobytes(), "little") * (pow(mr.R, -1, r) if form & 1 else 1) % r
                      for v in _host(vals)]
            full = caller.blind(L, R, vl, vr)
            assert np.array_equal(lr[j].reshape(2, 8), mr.pack_points(cv, full)), ("L, R", form, k, j)
            engine.ipa_fold(d_p, d_b, d_g, us[j], len=ln, form=form)
            caller.absorb(us[j])
            ln //= 2
        engine.sync(_stream())
        assert np.array_equal(cf[0], _host(d_p)[0]), ("c", form, k)
        assert np.array_equal(cf[1], mr.pack_scalars(form, [caller.f])[0]), ("f", form, k)


@pytest.mark.parametrize("form", [1, 3])
def test_long_rounds(engine, form):
    _run(engine, form, _case(form, 12))


@pytest.mark.parametrize("form", [1, 2])
def test_back_to_back_with_new_bases_and_an_msm_between(engine, form):
    cv = mr.curve_of_form(form)
    a, b = _case(form, 6, variant=1), _case(form, 7, variant=2)
    assert (a["U"], a["W"]) != (b["U"], b["W"])
    _run(engine, form, a)
    # a commitment between them: the scratch the rounds' Pippenger passes share
    n = 1 << 9
    gm, pts = mr.known_bases(form, n)
    rng = random.Random(77 + form)
    sc = [rng.randrange(mr.ORDER[cv]) for _ in range(n)]
    out = engine.msm(_dev(mr.pack_scalars(form, sc)).reshape(1, n, 4), _dev(mr.pack_points(cv, pts)), form=form)
    _run(engine, form, b)
    assert np.array_equal(_host(out).reshape(-1, 8), mr.pack_points(cv, [mr.expected_msm(form, sc, gm)]))
    _run(engine, form, a)  # and the first pair of bases again, from the cache or rebuilt
    # U = W: one table serves both
    c = dict(_case(form, 3, variant=3))
    c["wm"], c["W"] = c["um"], c["U"]
    t = tr.Transcript(cv)
    for pt in c["pre_pts"]:
        t.common_point(pt)
    for v in c["pre_vals"]:
        t.common_scalar(v)
    assert t.squeeze() == c["z"]
    c["want"] = tr.opening_known(cv, c["p"], ir.powers(cv, c["x"], c["n"]), c["gm"], c["um"], c["wm"], c["z"],
                                 c["rand"], t, c["f0"])
    c["state"] = np.array(t.words(), dtype=np.uint64)
    _run(engine, form, c)


@pytest.mark.parametrize("form", [0, 3])
def test_tensor_level_wrapper(engine, form):
    c = _case(form, 5)
    cv = c["cv"]
    d_p, d_g = _dev(mr.pack_scalars(form, c["p"])), _dev(mr.pack_points(cv, c["pts"]))
    state = engine.transcript_init()
    engine.transcript_absorb_points(state, _dev(mr.pack_points(cv, c["pre_pts"])), form=form)
    engine.transcript_absorb_scalars(state, _dev(mr.pack_scalars(form, c["pre_vals"])), form=form)
    z = engine.transcript_squeeze(state, form=form)
    d_b = engine.ipa_powers(c["x"], c["n"], form=form)
    f = _dev(mr.pack_scalars(form, [c["f0"]]))[0]
    lr, u, cf = engine.ipa_open(d_p, d_b, d_g, c["U"], c["W"], z, _dev(mr.pack_scalars(form, c["rand"])), state, f,
                                form=form)
    engine.sync(_stream())
    assert tuple(lr.shape) == (5, 2, 8) and tuple(u.shape) == (5, 4) and tuple(cf.shape) == (2, 4)
    _check(form, c, (_host(lr).reshape(5, 16), _host(u), _host(cf), _host(state), d_p, d_b, d_g))


def test_refused_arguments(engine):
    import torch

    from b2f import B2FError

    form, k = 1, 4
    c = _case(form, k)
    cv, n = c["cv"], c["n"]
    s = _stream()
    d_p0, d_g0 = _dev(mr.pack_scalars(form, c["p"])), _dev(mr.pack_points(cv, c["pts"]))
    d_b0 = engine.ipa_powers(c["x"], n, form=form)
    d_p, d_b, d_g = d_p0.clone(), d_b0.clone(), d_g0.clone()
    d_rand = _dev(mr.pack_scalars(form, c["rand"]))
    d_z = _dev(_limbs(c["z"]))
    state0 = engine.transcript_init()
    engine.transcript_absorb_points(state0, _dev(mr.pack_points(cv, c["pre_pts"])), form=form)
    engine.transcript_absorb_scalars(state0, _dev(mr.pack_scalars(form, c["pre_vals"])), form=form)
    engine.transcript_squeeze(state0, form=form)
    state = state0.clone()
    lr = torch.zeros((k, 16), dtype=torch.int64, device="cuda:0")
    u = torch.zeros((k, 4), dtype=torch.int64, device="cuda:0")
    cf = torch.zeros((2, 4), dtype=torch.int64, device="cuda:0")
    f0 = _dev(mr.pack_scalars(form, [c["f0"]]))[0]
    U, W = mr.pack_points(cv, [c["U"], c["W"]])
    ZERO = np.zeros(8, dtype=np.uint64)
    P, B, G, Z, RD, ST, LR, UU, CF = (t.data_ptr() for t in (d_p, d_b, d_g, d_z, d_rand, state, lr, u, cf))

    def good():
        d_p.copy_(d_p0)
        d_b.copy_(d_b0)
        d_g.copy_(d_g0)
        state.copy_(state0)
        cf[1].copy_(f0)
        engine.ipa_open_dev(P, B, G, n, U, W, Z, RD, ST, form, LR, UU, CF, s)
        engine.sync(s)
        _check(form, c, (_host(lr), _host(u), _host(cf), _host(state), d_p, d_b, d_g))

    good()
    ok = dict(p=P, b=B, g=G, n=n, U=U, W=W, z=Z, rand=RD, st=ST, form=form, lr=LR, u=UU, cf=CF)
    changes = [dict(p=0), dict(b=0), dict(g=0), dict(z=0), dict(rand=0), dict(st=0), dict(lr=0), dict(u=0),
               dict(cf=0),
               dict(p=P + 8), dict(b=B + 8), dict(g=G + 8), dict(z=Z + 8), dict(rand=RD + 8), dict(st=ST + 8),
               dict(lr=LR + 8), dict(u=UU + 8), dict(cf=CF + 8),
               dict(form=4), dict(n=0), dict(n=1), dict(n=3), dict(n=12), dict(n=1 << 29),
               dict(U=ZERO), dict(W=ZERO),
               dict(b=P + 32, n=2),                                  # the vectors on each other
               dict(lr=P), dict(lr=G + 64 * (n - 1)), dict(u=B), dict(cf=P + 32 * (n - 2)),   # an output on an input
               dict(lr=RD), dict(u=Z), dict(cf=RD + 32 * (2 * k - 1)),
               dict(lr=ST), dict(u=ST + 128), dict(cf=ST + 224),     # an output on the state
               dict(st=P), dict(st=RD), dict(st=G),          # the state on an input
               dict(u=LR + 128 * (k - 1)), dict(cf=LR), dict(cf=UU + 32 * (k - 1)), dict(lr=UU)]  # each other
    for ch in changes:
        a = dict(ok, **ch)
        engine.set_timing(True)
        with pytest.raises(B2FError) as e:
            engine.ipa_open_dev(a["p"], a["b"], a["g"], a["n"], a["U"], a["W"], a["z"], a["rand"], a["st"], a["form"],
                                a["lr"], a["u"], a["cf"], s)
        assert e.value.code == ERR_ARG, sorted(ch)
        times = engine.kernel_times()
        engine.set_timing(False)
        assert all(v[1] == 0 for v in times.values()), sorted(ch)
    good()
    # one good call is one region of the quotient kind
    d_p.copy_(d_p0)
    d_b.copy_(d_b0)
    d_g.copy_(d_g0)
    state.copy_(state0)
    cf[1].copy_(f0)
    engine.set_timing(True)
    engine.ipa_open_dev(P, B, G, n, U, W, Z, RD, ST, form, LR, UU, CF, s)
    times = engine.kernel_times()
    engine.set_timing(False)
    assert times["quotient"][1] == 1 and times["quotient"][0] > 0
    assert all(v[1] == 0 for kind, v in times.items() if kind != "quotient")
