"""Big-integer restatement of the inner product argument's opening rounds (halo2_proofs 0.3.0
poly/commitment/prover.rs::create_proof's loop, as the issue restates it), on tests/msm_ref.py.

    L = <p[half..], G[..half]>        R = <p[..half], G[half..]>
    value_l = <p[half..], b[..half]>  value_r = <p[..half], b[half..]>
    caller: L += [value_l z] U + [l_rand] W, the same for R; squeezes u
    p[i] += p[half+i] u^-1   b[i] += b[half+i] u   G[i] = G[i] + [u] G[half+i]
    caller: f += l_rand u^-1 + r_rand u

Two forms of the generator vector: affine points (round_points / fold_points: plain point
arithmetic, nothing known about the points), and KNOWN multiples g_i of the curve's generator
(round_known / fold_known: every expected point is a scalar mod r and one gen_mul), which is what
makes the expected values of a 2^13 round cheap. `Caller` is the host side of the loop: the U / W
terms, the blinding and f. Curves are indexed as in msm_ref (0 Vesta, 1 BN254 G1)."""
import random

import msm_ref as mr


def powers(cv, x, n):
    r = mr.ORDER[cv]
    out, v = [], 1
    for _ in range(n):
        out.append(v)
        v = v * x % r
    return out


def inner(cv, a, b):
    return sum(x * y for x, y in zip(a, b)) % mr.ORDER[cv]


def values(cv, p, b):
    """(value_l, value_r)"""
    half = len(p) // 2
    return inner(cv, p[half:], b[:half]), inner(cv, p[:half], b[half:])


def fold_scalars(cv, p, b, u):
    r = mr.ORDER[cv]
    half = len(p) // 2
    ui = pow(u, -1, r)
    return ([(p[i] + p[half + i] * ui) % r for i in range(half)],
            [(b[i] + b[half + i] * u) % r for i in range(half)])


# ---- generators as affine points --------------------------------------------------------------
def round_points(cv, p, G):
    """(L, R) by point arithmetic"""
    half = len(p) // 2
    return mr.bitwise_msm(cv, p[half:], G[:half]), mr.bitwise_msm(cv, p[:half], G[half:])


def fold_points(cv, G, u):
    half = len(G) // 2
    return [mr.add(cv, G[i], mr.mul(cv, u, G[half + i])) for i in range(half)]


# ---- generators as known multiples of the curve's generator -----------------------------------------
def round_known(cv, p, gm):
    """(l, r) with L = l Gen, R = r Gen"""
    half = len(p) // 2
    return inner(cv, p[half:], gm[:half]), inner(cv, p[:half], gm[half:])


def fold_known(cv, gm, u):
    r = mr.ORDER[cv]
    half = len(gm) // 2
    return [(gm[i] + u * gm[half + i]) % r for i in range(half)]


def points_of(cv, multiples):
    """affine points m Gen (None for m = 0 mod r)"""
    return [mr.gen_mul(cv, m % mr.ORDER[cv]) for m in multiples]


class Caller:
    """The host side of the loop: U, W (any points), z, the running f and the rounds' randomness."""

    def __init__(self, cv, U, W, z, f, seed):
        self.cv, self.U, self.W, self.z, self.f = cv, U, W, z, f
        self.rng = random.Random(seed)
        self.l_rand = self.r_rand = None

    def blind(self, L, R, value_l, value_r):
        """(L_full, R_full): what the transcript gets"""
        cv, r = self.cv, mr.ORDER[self.cv]
        self.l_rand, self.r_rand = self.rng.randrange(r), self.rng.randrange(r)
        full = []
        for pt, v, rnd in ((L, value_l, self.l_rand), (R, value_r, self.r_rand)):
            pt = mr.add(cv, pt, mr.mul(cv, v * self.z % r, self.U))
            full.append(mr.add(cv, pt, mr.mul(cv, rnd, self.W)))
        return full

    def absorb(self, u):
        r = mr.ORDER[self.cv]
        self.f = (self.f + self.l_rand * pow(u, -1, r) + self.r_rand * u) % r


def statement(cv, p, b, G, z, U, f, W):
    """Q = <p, G> + [z <p, b>] U + [f] W"""
    r = mr.ORDER[cv]
    q = mr.bitwise_msm(cv, p, G)
    q = mr.add(cv, q, mr.mul(cv, z * inner(cv, p, b) % r, U))
    return mr.add(cv, q, mr.mul(cv, f, W))


def opening_known(cv, p, x, gm, us):
    """A whole opening on known multiples: a list, per round, of
    dict(l, r, value_l, value_r, p, b, gm) -- the round's outputs and the folded vectors."""
    b = powers(cv, x, len(p))
    out = []
    for u in us:
        l, r_ = round_known(cv, p, gm)
        vl, vr = values(cv, p, b)
        p, b = fold_scalars(cv, p, b, u)
        gm = fold_known(cv, gm, u)
        out.append(dict(l=l, r=r_, value_l=vl, value_r=vr, p=p, b=b, gm=gm))
    return out
