"""tests/transcript_ref.py, the restatement the GPU transcript and one-call opening tests compare
with, tied to what it restates:

  1  the pure-Python BLAKE2b against hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript"),
     byte strings around the block edges, the explicit state (t, count, zero tail) on the way;
  2  the transcript's framing against hashlib with .copy() for the squeezes, on mixed sequences whose
     length at a squeeze's finalisation is 127, 128 and 129 bytes modulo 128 (one point, one scalar and
     thirty squeezes is exactly 128; the thirty-first is 129);
  3  the pure-Python opening, k = 1..5 on both curves by plain point arithmetic: it satisfies the
     argument's final identity (ipa_ref.statement) with the challenges re-derived from the L_j, R_j
     alone; the known-multiples form agrees with it; changing one L_j changes every later u.

Parity with a halo2 binary cannot be pinned here (no Rust toolchain): the framing is restated from
halo2_proofs 0.3.0 transcript.rs, as DESIGN.md §4.13 says. No GPU."""
import hashlib
import random

import pytest

import ipa_ref as ir
import msm_ref as mr
import transcript_ref as tr


def _hashlib():
    return hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1000])
def test_blake2b_matches_hashlib(n):
    rng = random.Random(n)
    data = bytes(rng.randrange(256) for _ in range(n))
    h = tr.Blake2b().update(data)
    want = _hashlib()
    want.update(data)
    assert h.digest() == want.digest()
    assert h.digest() == want.digest()  # a digest leaves the state alone
    # the explicit state: lazy last block, zero tail
    assert h.t + h.count == n and h.t % 128 == 0
    assert h.count == (n if n <= 128 else (n - 1) % 128 + 1)
    assert bytes(h.buf[h.count:]) == bytes(128 - h.count)
    w = h.words()
    assert len(w) == tr.STATE_WORDS and w[26] == h.count and w[27:] == [0] * 5


def test_blake2b_in_pieces_and_copies():
    rng = random.Random(7)
    data = bytes(rng.randrange(256) for _ in range(700))
    a, want = tr.Blake2b(), _hashlib()
    at = 0
    for step in (1, 127, 1, 128, 129, 3, 250, 61):
        a.update(data[at:at + step])
        want.update(data[at:at + step])
        at += step
        assert a.digest() == want.copy().digest(), at
        assert a.copy().update(b"xyz").digest() == hashlib.blake2b(
            data[:at] + b"xyz", digest_size=64, person=b"Halo2-Transcript").digest()
    assert at == 700
    assert tr.Blake2b(b"other").digest() != tr.Blake2b().digest()


def _framed(cv, steps):
    """Run `steps` on the restated transcript and on hashlib side by side -> the byte lengths at each
    squeeze's finalisation."""
    t, want, lengths, n = tr.Transcript(cv), _hashlib(), [], 0
    r, q = mr.ORDER[cv], mr.Q[cv]
    for kind, val in steps:
        if kind == "point":
            t.common_point(val)
            x, y = val if val is not None else (0, 0)
            want.update(b"\1" + x.to_bytes(32, "little") + y.to_bytes(32, "little"))
            assert val is None or (x < q and y < q)
            n += 65
        elif kind == "scalar":
            t.common_scalar(val)
            want.update(b"\2" + val.to_bytes(32, "little"))
            n += 33
        else:
            got = t.squeeze()
            want.update(b"\0")
            n += 1
            fin = want.copy()
            assert got == int.from_bytes(fin.digest(), "little") % r
            lengths.append(n)
        assert t.hash.t + t.hash.count == n
    return lengths


@pytest.mark.parametrize("cv", [0, 1])
def test_framing_at_the_block_edges(cv):
    rng = random.Random(40 + cv)
    pt = mr.gen_mul(cv, rng.randrange(1, mr.ORDER[cv]))
    s = rng.randrange(mr.ORDER[cv])
    # 65 + 33 + 30 squeezes = 128 bytes at the thirtieth squeeze, 129 at the thirty-first
    lengths = _framed(cv, [("point", pt), ("scalar", s)] + [("squeeze", None)] * 31)
    assert lengths[28:31] == [127, 128, 129]
    # the same edges a block later, points and scalars mixed with the squeezes; the identity too
    steps = [("point", pt), ("squeeze", None), ("scalar", s), ("point", None), ("scalar", 0),
             ("scalar", mr.ORDER[cv] - 1)]  # 65 + 1 + 33 + 65 + 33 + 33 = 230
    steps += [("squeeze", None)] * 27       # 255, 256, 257 at the last three
    lengths = _framed(cv, steps)
    assert [x % 128 for x in lengths[-3:]] == [127, 0, 1] and lengths[-1] == 257


def _opening_case(cv, k, seed):
    rng = random.Random(seed)
    r = mr.ORDER[cv]
    n = 1 << k
    p = [rng.randrange(r) for _ in range(n)]
    x = rng.randrange(1, r)
    gm = [rng.randrange(1, r) for _ in range(n)]
    um, wm = rng.randrange(1, r), rng.randrange(1, r)
    rand = [rng.randrange(r) for _ in range(2 * k)]
    f0 = rng.randrange(r)
    t = tr.Transcript(cv)
    t.common_point(mr.gen_mul(cv, rng.randrange(1, r)))
    t.common_scalar(rng.randrange(r))
    z = t.squeeze()
    return dict(p=p, b=ir.powers(cv, x, n), gm=gm, um=um, wm=wm, rand=rand, f0=f0, t=t, z=z)


@pytest.mark.parametrize("cv", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_opening_satisfies_the_final_identity(cv, k):
    c = _opening_case(cv, k, 100 * cv + k)
    r = mr.ORDER[cv]
    G = ir.points_of(cv, c["gm"])
    U, W = mr.gen_mul(cv, c["um"]), mr.gen_mul(cv, c["wm"])
    start = c["t"].copy()
    out = tr.opening_points(cv, c["p"], c["b"], G, U, W, c["z"], c["rand"], c["t"], c["f0"])
    assert len(out["lr"]) == len(out["u"]) == k and len(out["p"]) == len(out["b"]) == len(out["g"]) == 1
    # the known-multiples form is the same opening
    known = tr.opening_known(cv, c["p"], c["b"], c["gm"], c["um"], c["wm"], c["z"], c["rand"], start.copy(),
                             c["f0"])
    assert known["lr"] == out["lr"] and known["u"] == out["u"] and (known["c"], known["f"]) == (out["c"], out["f"])
    assert ir.points_of(cv, known["g"]) == out["g"]
    # a verifier's view: the challenges from L_j, R_j alone, then the final identity
    v = start.copy()
    us = []
    for L, R in out["lr"]:
        v.common_point(L)
        v.common_point(R)
        us.append(v.squeeze())
    assert us == out["u"]
    v.common_scalar(out["c"])
    v.common_scalar(out["f"])
    assert v.words() == c["t"].words()
    # Q' = Q + sum_j (u_j^-1 L_j + u_j R_j) = [c] G' + [c b' z] U + [f] W
    q = ir.statement(cv, c["p"], c["b"], G, c["z"], U, c["f0"], W)
    for (L, R), u in zip(out["lr"], us):
        q = mr.add(cv, q, mr.add(cv, mr.mul(cv, pow(u, -1, r), L), mr.mul(cv, u, R)))
    assert q == ir.statement(cv, [out["c"]], out["b"], out["g"], c["z"], U, out["f"], W)


@pytest.mark.parametrize("cv", [0, 1])
def test_one_changed_l_changes_every_later_challenge(cv):
    k = 5
    c = _opening_case(cv, k, 900 + cv)
    start = c["t"].copy()
    out = tr.opening_known(cv, c["p"], c["b"], c["gm"], c["um"], c["wm"], c["z"], c["rand"], c["t"], c["f0"])
    for changed in range(k):
        v, us = start.copy(), []
        for j, (L, R) in enumerate(out["lr"]):
            v.common_point(mr.add(cv, L, mr.GEN[cv]) if j == changed else L)
            v.common_point(R)
            us.append(v.squeeze())
        assert us[:changed] == out["u"][:changed]
        assert all(a != b for a, b in zip(us[changed:], out["u"][changed:])), changed
