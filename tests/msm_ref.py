"""Big-integer reference of the commitment curves and the multi-scalar multiplication, with its
own constants (nothing imported from the package): Jacobian addition and doubling for a = 0, scalar
multiplication, a naive MSM, and bases that are KNOWN multiples of the generator, so that the
expected MSM of a large case is one scalar multiplication: sum s_i (b_i G) = (sum s_i b_i mod r) G.

Curves are indexed 0 (Vesta, forms 0/1) and 1 (BN254 G1, forms 2/3). Affine points are (x, y)
tuples of ints, the identity None."""
import random

import numpy as np

# base-field modulus, b, group order (= the scalar field's modulus), generator
Q = (0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
     0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47)
B = (5, 3)
ORDER = (0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
         0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001)
GEN = ((Q[0] - 1, 2), (1, 2))
R = 1 << 256


def curve_of_form(form):
    return (form >> 1) & 1


def on_curve(cv, pt):
    if pt is None:
        return True
    x, y = pt
    return (y * y - x * x * x - B[cv]) % Q[cv] == 0


# Jacobian (X, Y, Z), the identity Z = 0
def jac_double(cv, p):
    q = Q[cv]
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    A = X * X % q
    Bv = Y * Y % q
    C = Bv * Bv % q
    D = 2 * ((X + Bv) * (X + Bv) - A - C) % q
    E = 3 * A % q
    X3 = (E * E - 2 * D) % q
    Y3 = (E * (D - X3) - 8 * C) % q
    Z3 = 2 * Y * Z % q
    return (X3, Y3, Z3)


def jac_add(cv, p1, p2):
    q = Q[cv]
    X1, Y1, Z1 = p1
    X2, Y2, Z2 = p2
    if Z1 == 0:
        return p2
    if Z2 == 0:
        return p1
    Z1Z1 = Z1 * Z1 % q
    Z2Z2 = Z2 * Z2 % q
    U1 = X1 * Z2Z2 % q
    U2 = X2 * Z1Z1 % q
    S1 = Y1 * Z2 * Z2Z2 % q
    S2 = Y2 * Z1 * Z1Z1 % q
    H = (U2 - U1) % q
    r = (S2 - S1) % q
    if H == 0:
        return jac_double(cv, p1) if r == 0 else (1, 1, 0)
    HH = H * H % q
    HHH = H * HH % q
    V = U1 * HH % q
    X3 = (r * r - HHH - 2 * V) % q
    Y3 = (r * (V - X3) - S1 * HHH) % q
    Z3 = Z1 * Z2 * H % q
    return (X3, Y3, Z3)


def to_jac(pt):
    return (1, 1, 0) if pt is None else (pt[0], pt[1], 1)


def to_affine(cv, p):
    q = Q[cv]
    X, Y, Z = p
    if Z == 0:
        return None
    zi = pow(Z, -1, q)
    return (X * zi * zi % q, Y * zi * zi * zi % q)


def batch_affine(cv, ps):
    """Jacobian points (none the identity) -> affine, with one inversion."""
    q = Q[cv]
    pref = [1]
    for p in ps:
        assert p[2] != 0
        pref.append(pref[-1] * p[2] % q)
    inv = pow(pref[-1], -1, q)
    out = [None] * len(ps)
    for i in range(len(ps) - 1, -1, -1):
        zi = inv * pref[i] % q
        inv = inv * ps[i][2] % q
        X, Y, _ = ps[i]
        zi2 = zi * zi % q
        out[i] = (X * zi2 % q, Y * zi2 * zi % q)
    return out


def neg(cv, pt):
    return None if pt is None else (pt[0], (-pt[1]) % Q[cv])


def add(cv, a, b):
    return to_affine(cv, jac_add(cv, to_jac(a), to_jac(b)))


def double(cv, a):
    return to_affine(cv, jac_double(cv, to_jac(a)))


def jac_mul(cv, k, pt):
    acc = (1, 1, 0)
    base = to_jac(pt)
    for bit in bin(k)[2:] if k else "":
        acc = jac_double(cv, acc)
        if bit == "1":
            acc = jac_add(cv, acc, base)
    return acc


def mul(cv, k, pt):
    """k pt for any integer k >= 0 (not reduced: r G = identity is a test)."""
    return to_affine(cv, jac_mul(cv, k, pt))


def naive_msm(cv, scalars, points):
    acc = (1, 1, 0)
    for s, p in zip(scalars, points):
        acc = jac_add(cv, acc, jac_mul(cv, s, p))
    return to_affine(cv, acc)


def bitwise_msm(cv, scalars, points):
    """The same sum with the doublings shared (bit by bit from the top, every point whose scalar
    has the bit added): a third of naive_msm's cost, and as independent of known multiples."""
    acc = (1, 1, 0)
    js = [to_jac(p) for p in points]
    top = max([s.bit_length() for s in scalars] + [0])
    for bit in range(top - 1, -1, -1):
        acc = jac_double(cv, acc)
        for s, p in zip(scalars, js):
            if (s >> bit) & 1:
                acc = jac_add(cv, acc, p)
    return to_affine(cv, acc)


# ---- bases that are known multiples of the generator ---------------------------------------------
_TABLE = {}
_POOL = {}
_FAMILY = {}
POOL_SIZE = 1024


def _table(cv):
    """Fixed-base table of G: t[j][d] = d 256^j G (Jacobian), 32 x 256 entries."""
    if cv not in _TABLE:
        rows = []
        base = to_jac(GEN[cv])
        for _ in range(32):
            row = [(1, 1, 0), base]
            for _ in range(254):
                row.append(jac_add(cv, row[-1], base))
            rows.append(row)
            base = jac_add(cv, row[-1], base)  # 256 base
        _TABLE[cv] = rows
    return _TABLE[cv]


def gen_mul(cv, k):
    """k G (affine) for 0 <= k < 2^256 from the fixed-base table."""
    t = _table(cv)
    acc = (1, 1, 0)
    for j in range(32):
        d = (k >> (8 * j)) & 255
        if d:
            acc = jac_add(cv, acc, t[j][d])
    return to_affine(cv, acc)


def pool(cv):
    """(multiples b_i, points b_i G): POOL_SIZE random multiples, built once per process."""
    if cv not in _POOL:
        rng = random.Random(1000 + cv)
        t = _table(cv)
        bs = [rng.randrange(1, ORDER[cv]) for _ in range(POOL_SIZE)]
        js = []
        for k in bs:
            acc = (1, 1, 0)
            for j in range(32):
                d = (k >> (8 * j)) & 255
                if d:
                    acc = jac_add(cv, acc, t[j][d])
            js.append(acc)
        _POOL[cv] = (bs, batch_affine(cv, js))
    return _POOL[cv]


def family(cv, n):
    """(b_i, points) with b_i = b_0 + i d: one mixed addition per point, one batched inversion."""
    if cv not in _FAMILY or len(_FAMILY[cv][0]) < n:  # a longer family's prefix serves a shorter one
        rng = random.Random(2000 + cv)
        b0, d = rng.randrange(1, ORDER[cv]), rng.randrange(1, ORDER[cv])
        step = to_jac(gen_mul(cv, d))
        cur = to_jac(gen_mul(cv, b0))
        js = []
        for _ in range(n):
            js.append(cur)
            cur = jac_add(cv, cur, step)
        _FAMILY[cv] = ([(b0 + i * d) % ORDER[cv] for i in range(n)], batch_affine(cv, js))
    bs, ps = _FAMILY[cv]
    return bs[:n], ps[:n]


def known_bases(form, n, incremental=False):
    """(b, points): n affine points b_i G of the form's curve with their multiples b_i. The pool
    (n <= POOL_SIZE, or cycled beyond it) or the incremental family."""
    cv = curve_of_form(form)
    if incremental:
        return family(cv, n)
    bs, ps = pool(cv)
    return [bs[i % POOL_SIZE] for i in range(n)], [ps[i % POOL_SIZE] for i in range(n)]


def expected_msm(form, scalars, multiples):
    """(sum s_i b_i mod r) G."""
    cv = curve_of_form(form)
    k = sum(s * b for s, b in zip(scalars, multiples)) % ORDER[cv]
    return gen_mul(cv, k)


# ---- the device layouts ----------------------------------------------------------------------------
def pack_points(cv, pts):
    """Affine points -> uint64 [n, 8], coordinates in base-field Montgomery form; None -> zeros."""
    q = Q[cv]
    raw = bytearray()
    for pt in pts:
        if pt is None:
            raw += bytes(64)
        else:
            raw += (pt[0] * R % q).to_bytes(32, "little") + (pt[1] * R % q).to_bytes(32, "little")
    return np.frombuffer(bytes(raw), dtype=np.uint64).reshape(-1, 8).copy()


def unpack_points(cv, limbs):
    q = Q[cv]
    rinv = pow(R, -1, q)
    raw = np.ascontiguousarray(limbs).view(np.uint64).reshape(-1, 8).tobytes()
    out = []
    for i in range(0, len(raw), 64):
        x = int.from_bytes(raw[i:i + 32], "little")
        y = int.from_bytes(raw[i + 32:i + 64], "little")
        out.append(None if x == 0 and y == 0 else (x * rinv % q, y * rinv % q))
    return out


def pack_scalars(form, vals):
    """Scalars (ints < r) -> uint64 [n, 4] in `form` (bit 0: Montgomery)."""
    r = ORDER[curve_of_form(form)]
    if form & 1:
        vals = [v * R % r for v in vals]
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals),
                         dtype=np.uint64).reshape(-1, 4).copy()
