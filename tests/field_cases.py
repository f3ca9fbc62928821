"""Operands for the field-primitive tests, shared by tests/test_gpu_field.py (the device code
through b2f_debug_field_op) and tests/test_mont_asm_gen.py (the CPU interpreter of the generated
product): the edge set E and products crafted to have a chosen Montgomery reduction word.

A Montgomery product a b / R (R = 2^256, 32-bit words) adds m p to a b with
m = a b (-p^-1) mod R; the column-k reduction word m_k of product scanning is word k of m. A random
product has m_k in {0, 0xffffffff} with probability 2^-31 per column, so the paths those words
take are built here instead: choose m with word k = v and a random odd a < p, then
b = m (-p) a^-1 mod R gives a b (-p^-1) = m mod R exactly; a is redrawn until b < p."""
import random

import numpy as np

P_PALLAS = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
P_BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MODULI = (P_PALLAS, P_BN254)  # indexed by the probe's field argument
R = 1 << 256
M32 = 0xffffffff

CRAFT_WORDS = (0, 1, 0x80000000, 0xfffffffe, 0xffffffff)
CRAFT_FILLS = ("random", "zero", "ones", "low_zero", "random2", "random3")
CRAFT_TARGETS = 8 * len(CRAFT_WORDS) * len(CRAFT_FILLS)  # 240 per field
CRAFT_DRAWS = 200
CRAFT_MIN_FOUND = CRAFT_TARGETS - CRAFT_TARGETS * 5 // 100  # at most 5 % without a pair


def edge_set(p):
    """E: every value is below p (both moduli are above 2^253)."""
    top = p >> 224
    e = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, 1 << 16, (1 << 32) - 1,
         1 << 32, (1 << 64) - 1, 1 << 128, 1 << 224, 1 << 253,
         ((top - 1) << 224) + (1 << 224) - 1]  # every low word all ones
    assert all(0 <= v < p for v in e) and len(set(e)) == len(e) == 17
    return e


def edge_pairs(p):
    e = edge_set(p)
    return [(a, b) for a in e for b in e]


def _craft_m(rng, k, v, fill):
    if fill == "zero":
        words = [0] * 8
    elif fill == "ones":
        words = [M32] * 8
    else:
        words = [rng.getrandbits(32) for _ in range(8)]
        if fill == "low_zero":
            words[:k] = [0] * k
    words[k] = v
    return sum(w << (32 * i) for i, w in enumerate(words))


def crafted_pairs(p, seed=11):
    """[(k, v, fill, a, b)] for the targets that got a pair, in target order; len() is the count
    found out of CRAFT_TARGETS. Every pair has a, b < p and a b (-p^-1) mod R == m with word k of
    m equal to v (asserted here)."""
    rng = random.Random(seed)
    negp = R - p
    negpinv = pow(negp, -1, R)
    out = []
    for k in range(8):
        for v in CRAFT_WORDS:
            for fill in CRAFT_FILLS:
                for _ in range(CRAFT_DRAWS):
                    m = _craft_m(rng, k, v, fill)
                    a = rng.randrange(1, p, 2)  # odd: invertible mod R
                    b = m * negp * pow(a, -1, R) % R
                    if b < p:
                        got = a * b * negpinv % R
                        assert got == m and (got >> (32 * k)) & M32 == v
                        out.append((k, v, fill, a, b))
                        break
    return out


CARRY_PER_COLUMN = 4
CARRY_TARGETS = 7 * CARRY_PER_COLUMN  # columns 1..7
CARRY_MIN_FOUND = CARRY_TARGETS - CARRY_TARGETS * 5 // 100


def column_sum(p, a, b, k):
    """The accumulator of product scanning at the end of column k <= 7, before m_k p_0 is added:
    (carry from the columns below) + sum a_i b_(k-i) + sum_(i<k) m_i p_(k-i), as an integer."""
    aw = [(a >> (32 * i)) & M32 for i in range(8)]
    bw = [(b >> (32 * i)) & M32 for i in range(8)]
    pw = [(p >> (32 * i)) & M32 for i in range(8)]
    npw = pow(R - p, -1, 1 << 32)
    acc, m = 0, []
    for col in range(k + 1):
        acc += sum(aw[i] * bw[col - i] for i in range(col + 1))
        acc += sum(m[i] * pw[col - i] for i in range(col))
        if col == k:
            return acc
        m.append(acc * npw & M32)
        acc += m[col] * pw[0]
        assert acc & M32 == 0
        acc >>= 32


def carry_pairs(p, seed=12):
    """[(k, a, b)]: products whose column-k accumulator (k = 1..7) ends with a non-zero low word
    and a high word of 2^32 - 1, so that cancelling the low word carries through the whole high
    word into the carry word (pallas: the v_sub_co borrow added to ACC.hi at the column shift). A
    random product does that with probability 2^-32 per column. b_k enters column k only through
    a_0 b_k, so with everything else drawn at random b_k is solved for: the window of 2^32 values
    of the accumulator's low 64 bits holds a multiple of a_0 < 2^32."""
    rng = random.Random(seed)
    out = []
    for k in range(1, 8):
        found = 0
        for _ in range(CRAFT_DRAWS):
            if found == CARRY_PER_COLUMN:
                break
            a = rng.randrange(p) | (1 << 31)  # a_0 >= 2^31: b_k = ceil(D / a_0) fits a word
            b = rng.randrange(p) & ~(M32 << (32 * k))
            if a >= p:
                continue
            c = column_sum(p, a, b, k)
            d = ((M32 << 32) - c) % (1 << 64)
            bk = -(-d // (a & M32))
            if bk > M32:
                continue
            b |= bk << (32 * k)
            v = column_sum(p, a, b, k)
            if b >= p or (v >> 32) & M32 != M32 or v & M32 == 0:
                continue
            out.append((k, a, b))
            found += 1
    return out


def pack(vals):
    """ints < 2^256 as uint64 [len, 4] little-endian limbs, as given (no form conversion)."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals),
                         dtype=np.uint64).reshape(-1, 4).copy()


def unpack(limbs):
    raw = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
