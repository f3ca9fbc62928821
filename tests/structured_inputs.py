"""Structured compression inputs: whole-word extremes that uniform draws reach with probability
2^-64, shared by tests/test_structured_inputs_ref.py (CPU) and tests/test_gpu_structured_inputs.py.
Nothing here touches the GPU.

  f_ref     RFC 7693 section 3.2 / EIP-152 `F` on Python integers, written from the RFC.
  g_trace   the same function one G half at a time, every intermediate word kept.
  batch     a deterministic INPUT_DTYPE array of 2,002 instances: 14 x 14 broadcast word patterns
            for h x m, ten (t, f, rounds) variants of each (1,960), and 16 solved or all-extreme
            instances placed twice each (index 0, indices 191..765; 1,520..1,926 and the last
            index), five of them twice more (900..1,377), each between pattern instances.
  census    the blocks of a trace, by class, whose 64-bit word sits at an extreme: found from the
            fixed column's selector bits and the cells alone.
  expected_census  the same counts from g_trace on the inputs, without a trace.

The solved instances come from column 0 of round 0: a = h_0, b = h_4, c = IV_0, d = IV_4 ^ t_0,
x = m[SIGMA[0][0]] = m_0, y = m[SIGMA[0][1]] = m_1 (column 1: h_1, h_5, IV_1, IV_5 ^ t_1, m_2).
h_0, h_4 and m_0 set the first ADD3's sum, t_0 then moves d freely, so the first XOR's output and
(through the rot-32) the first ADD2's result and the XOR24's output are free; m_1 sets the second
ADD3's sum and through it the XOR63's output.

Two targets one might ask for do not exist, by arithmetic:
  * an ADD3 with result all ones and carry 2: the largest sum is 3 (2^64 - 1) = 2 * 2^64 +
    (2^64 - 3), so with carry 2 the result is at most 2^64 - 3. The batch holds that largest sum
    (a = b = m = 2^64 - 1: `add3_max`) and the all-ones result with carry 1 (`add3_ones`).
  * an f = 1 instance whose v_14 before the complement is all ones: v_14 before the complement is
    the constant IV_6. The batch holds f = 1 instances in which the complemented v_14 meets an
    `a` that makes column 2's first XOR output all ones, and all zeros (`f1_xor_ones`,
    `f1_xor_zero`).
"""
import numpy as np

M64 = (1 << 64) - 1
IV = (0x6A09E667F3BCC908, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1,
      0x510E527FADE682D1, 0x9B05688C2B3E6C1F, 0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179)
SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
         (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
         (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4),
         (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
         (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13),
         (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
         (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11),
         (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
         (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5),
         (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
G_INDEX = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
           (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))
ROT = ((32, 24), (16, 63))  # (d, b) rotations of the first and the second half of G

INIT_ROWS, ROUND_ROWS, FINAL_ROWS = 164, 416, 64
PAD_ROWS = 8  # zero rows past the batch in the reference trace


def rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def rotl(x, n):
    return rotr(x, 64 - n)


def f_ref(rounds, h, m, t, f):
    """h' of one compression (RFC 7693 section 3.2 with EIP-152's explicit round count)."""
    h = [int(w) for w in h]
    m = [int(w) for w in m]
    v = h + list(IV)
    v[12] ^= int(t[0])
    v[13] ^= int(t[1])
    if int(f):
        v[14] ^= M64

    def mix(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & M64
        v[d] = rotr(v[d] ^ v[a], 32)
        v[c] = (v[c] + v[d]) & M64
        v[b] = rotr(v[b] ^ v[c], 24)
        v[a] = (v[a] + v[b] + y) & M64
        v[d] = rotr(v[d] ^ v[a], 16)
        v[c] = (v[c] + v[d]) & M64
        v[b] = rotr(v[b] ^ v[c], 63)

    for r in range(int(rounds)):
        s = SIGMA[r % 10]
        for g, (a, b, c, d) in enumerate(G_INDEX):
            mix(a, b, c, d, m[s[2 * g]], m[s[2 * g + 1]])
    return [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]


def g_trace(rounds, h, m, t, f):
    """(init, halves, h'): `init` the three words v_12, v_13, v_14 after the t / f mix (the outputs
    of the init region's XOR blocks), `halves` one record per G half in trace order:
    (round, g, half, add3_sum, xor_d, add2_sum, xor_b) -- add3_sum = a + b + x and add2_sum = c + d
    as unreduced integers (result = sum mod 2^64, carry = sum >> 64), xor_d = d ^ a and xor_b =
    b ^ c before their rotations."""
    h = [int(w) for w in h]
    m = [int(w) for w in m]
    v = h + list(IV)
    v[12] ^= int(t[0])
    v[13] ^= int(t[1])
    if int(f):
        v[14] ^= M64
    init = (v[12], v[13], v[14])
    halves = []
    for r in range(int(rounds)):
        s = SIGMA[r % 10]
        for g, (a, b, c, d) in enumerate(G_INDEX):
            for half in (0, 1):
                s3 = v[a] + v[b] + m[s[2 * g + half]]
                v[a] = s3 & M64
                xd = v[d] ^ v[a]
                v[d] = rotr(xd, ROT[half][0])
                s2 = v[c] + v[d]
                v[c] = s2 & M64
                xb = v[b] ^ v[c]
                v[b] = rotr(xb, ROT[half][1])
                halves.append((r, g, half, s3, xd, s2, xb))
    return init, halves, [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]


# ------------------------------------------------------------------------------ the batch
PATTERNS = (0, M64, 1, 2, 1 << 63, M64 - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA,
            0x0000FFFF0000FFFF, 0xFFFF0000FFFF0000, 0x00FF00FF00FF00FF, 0x7FFF7FFF7FFF7FFF,
            0x8000800080008000, 0x0100010001000100)
ROUNDS = (0, 1, 2, 10, 12, 13)  # 12 and 13: SIGMA[r mod 10] wraps
VARIANTS = 10  # (t kind, f, rounds) variants per (h, m) pattern pair
T_KINDS = ("zero", "ones", "h^m", "iv")


def _t_words(kind, hp, mp):
    return {"zero": (0, 0), "ones": (M64, M64), "h^m": (hp ^ mp, hp ^ mp), "iv": (IV[4], IV[5])}[kind]


def _free(seed):
    """Fixed, unremarkable words for the fields a solved instance leaves free."""
    w = lambda k: (0x9E3779B97F4A7C15 * (seed * 40 + k + 1) + 0xC2B2AE3D27D4EB4F) & M64  # noqa: E731
    return [w(k) for k in range(8)], [w(8 + k) for k in range(16)], [w(24), w(25)]


def _solve(name):
    """(h, m, t, f) of the solved instance `name`; each is checked against g_trace by
    solved_ok()."""
    h, m, t = _free(sorted(SOLVED).index(name))
    f = 0
    if name == "all_extreme":
        return [M64] * 8, [M64] * 16, [M64, M64], 1
    if name == "add3_zero_c2":
        h[0], h[4], m[0] = M64, M64, 2
    elif name == "add3_zero_c1":
        h[0] &= M64 >> 2
        h[4] &= M64 >> 2
        m[0] = (1 << 64) - h[0] - h[4]
    elif name == "add3_max":
        h[0], h[4], m[0] = M64, M64, M64
    elif name == "add3_ones":
        h[0], h[4], m[0] = M64, M64, 1
    a1 = (h[0] + h[4] + m[0]) & M64
    if name == "xor_zero":
        t[0] = IV[4] ^ a1
    elif name == "xor_ones":
        t[0] = IV[4] ^ a1 ^ M64
    elif name == "add2_zero_c1":  # d = 2^64 - IV_0 after the rot-32
        t[0] = IV[4] ^ a1 ^ rotl((1 << 64) - IV[0], 32)
    elif name == "add2_ones":
        t[0] = IV[4] ^ a1 ^ rotl(M64 - IV[0], 32)
    elif name == "add2_zero_c1_col1":
        t[1] = IV[5] ^ ((h[1] + h[5] + m[2]) & M64) ^ rotl((1 << 64) - IV[1], 32)
    elif name in ("xor24_zero", "xor24_ones"):  # c = b (or ~b) after the first ADD2
        c1 = h[4] if name == "xor24_zero" else h[4] ^ M64
        t[0] = IV[4] ^ a1 ^ rotl((c1 - IV[0]) & M64, 32)
    elif name in ("xor63_zero", "xor63_ones"):  # c = b (or ~b) after the second ADD2, through m_1
        d1 = rotr(IV[4] ^ t[0] ^ a1, 32)
        c1 = (IV[0] + d1) & M64
        b1 = rotr(h[4] ^ c1, 24)
        c2 = b1 if name == "xor63_zero" else b1 ^ M64
        a2 = d1 ^ rotl((c2 - c1) & M64, 16)
        m[1] = (a2 - a1 - b1) & M64
    elif name in ("f1_xor_ones", "f1_xor_zero"):  # column 2: d = ~IV_6, a = h_2 + h_6 + m_4
        f = 1
        want = IV[6] if name == "f1_xor_ones" else IV[6] ^ M64
        m[4] = (want - h[2] - h[6]) & M64
    return h, m, t, f


# name -> (column, half, what must hold of that half's record in round 0)
SOLVED = {
    "all_extreme": None,
    "add3_zero_c2": (0, 0, lambda s3, xd, s2, xb: s3 == 2 << 64),
    "add3_zero_c1": (0, 0, lambda s3, xd, s2, xb: s3 == 1 << 64),
    "add3_max": (0, 0, lambda s3, xd, s2, xb: s3 == 3 * M64),
    "add3_ones": (0, 0, lambda s3, xd, s2, xb: s3 == (1 << 64) + M64),
    "xor_zero": (0, 0, lambda s3, xd, s2, xb: xd == 0),
    "xor_ones": (0, 0, lambda s3, xd, s2, xb: xd == M64),
    "add2_zero_c1": (0, 0, lambda s3, xd, s2, xb: s2 == 1 << 64),
    "add2_ones": (0, 0, lambda s3, xd, s2, xb: s2 == M64),
    "add2_zero_c1_col1": (1, 0, lambda s3, xd, s2, xb: s2 == 1 << 64),
    "xor24_zero": (0, 0, lambda s3, xd, s2, xb: xb == 0),
    "xor24_ones": (0, 0, lambda s3, xd, s2, xb: xb == M64),
    "xor63_zero": (0, 1, lambda s3, xd, s2, xb: xb == 0),
    "xor63_ones": (0, 1, lambda s3, xd, s2, xb: xb == M64),
    "f1_xor_ones": (2, 0, lambda s3, xd, s2, xb: xd == M64),
    "f1_xor_zero": (2, 0, lambda s3, xd, s2, xb: xd == 0),
}
SPECIALS = tuple(SOLVED)  # placement order
N_PATTERN = len(PATTERNS) ** 2 * VARIANTS  # 1,960
# the targets no pattern instance reaches get two more placements, so that their census classes
# hold four blocks
RARE = ("add2_ones", "xor24_zero", "xor24_ones", "xor63_zero", "xor63_ones")
N_BATCH = N_PATTERN + 2 * len(SPECIALS) + 2 * len(RARE)  # 2,002
# where the specials sit: the first index, the hundreds; past 1,500, the last index; the extra
# placements of the rare ones between them
FIRST_AT = tuple([0] + [150 + 41 * i for i in range(1, len(SPECIALS))])
SECOND_AT = tuple([1520 + 29 * i for i in range(len(SPECIALS) - 1)] + [N_BATCH - 1])
THIRD_AT = tuple(900 + 53 * i for i in range(2 * len(RARE)))
FIRST_ROUNDS = (1, 2)  # the first placement alternates these, the second 12 and 13
SECOND_ROUNDS = (12, 13)
THIRD_ROUNDS = (10, 13)  # a rare one's third and fourth placement


def placements():
    """[(index in batch(), name, rounds)] of the solved and all-extreme instances."""
    out = []
    for k, name in enumerate(SPECIALS):
        out.append((FIRST_AT[k], name, FIRST_ROUNDS[k % 2]))
        out.append((SECOND_AT[k], name, SECOND_ROUNDS[k % 2]))
    for k, name in enumerate(RARE):
        for j in (0, 1):
            out.append((THIRD_AT[2 * k + j], name, THIRD_ROUNDS[j]))
    assert len({p[0] for p in out}) == len(out) == N_BATCH - N_PATTERN
    return sorted(out)


def solved_ok(name):
    """The solved instance `name` reaches its target, by g_trace."""
    if SOLVED[name] is None:
        return True
    col, half, ok = SOLVED[name]
    h, m, t, f = _solve(name)
    _, halves, _ = g_trace(1, h, m, t, f)
    rec = next(x for x in halves if x[:3] == (0, col, half))
    return bool(ok(*rec[3:]))


def _input_dtype():
    import oracle

    return oracle.INPUT_DTYPE


_batch = None


def special_positions():
    """{index in batch(): name of the solved or all-extreme instance there}."""
    return {i: name for i, name, _ in placements()}


def batch():
    """The structured batch (a copy; the layout is fixed and deterministic)."""
    global _batch
    if _batch is None:
        recs = []
        for ih, hp in enumerate(PATTERNS):
            for im, mp in enumerate(PATTERNS):
                pair = ih * len(PATTERNS) + im
                for j in range(VARIANTS):
                    t = _t_words(T_KINDS[j % 4], hp, mp)
                    recs.append(([hp] * 8, [mp] * 16, list(t), (j // 4) & 1,
                                 ROUNDS[(pair + j) % len(ROUNDS)]))
        assert len(recs) == N_PATTERN
        special = {i: (name, rounds) for i, name, rounds in placements()}
        x = np.zeros(N_BATCH, dtype=_input_dtype())
        it = iter(recs)
        for i in range(N_BATCH):
            if i in special:
                name, rounds = special[i]
                h, m, t, f = _solve(name)
            else:
                h, m, t, f, rounds = next(it)
            x["h"][i] = np.array(h, dtype=np.uint64)
            x["m"][i] = np.array(m, dtype=np.uint64)
            x["t"][i] = np.array(t, dtype=np.uint64)
            x["f"][i] = f
            x["rounds"][i] = rounds
        assert next(it, None) is None
        _batch = x
    return _batch.copy()


# ------------------------------------------------------------------------------ the census
WORD_CLASSES = ("add3_zero_c1", "add2_zero_c1", "add3_zero_c2", "add3_ones", "add2_ones",
                "xor_zero", "xor_ones", "xor24_zero", "xor24_ones", "xor63_zero", "xor63_ones")
PIECE_CLASSES = ("xor63_zb1_7fff", "xor24_ff_tag0")
CLASSES = WORD_CLASSES + PIECE_CLASSES
# class -> (row stride between the block's four limb rows, whether a_9 of its first row is a carry)
CLASS_SHAPE = {c: ((1, True) if c.startswith("add") else (3, False) if c.startswith("xor24")
                   else (2, False)) for c in CLASSES}

_BITS = {"add3": (1 << 3) | (1 << 7), "add2": (1 << 5) | (1 << 9),
         "xor": (1 << 6) | (1 << 10) | (1 << 12), "xor24": 1 << 4, "xor63": 1 << 8}


def _starts(fixed, kind):
    return np.flatnonzero(fixed & np.uint32(_BITS[kind]))


def _word(limbs):
    """uint64 words of four uint64 limb arrays."""
    return limbs[0] | (limbs[1] << np.uint64(16)) | (limbs[2] << np.uint64(32)) | (limbs[3] << np.uint64(48))


def census(adv, fixed):
    """{class: the first rows (ascending) of the blocks in it}, from the selector bits of `fixed`
    and the cells of `adv` ([10, rows] u32) alone. A block's word is recomposed from its dense
    lookup cells as docs/LAYOUT.md section 4 lays them out: ADD a_1@k; XOR a_1@2k; XOR24 a_1@3k |
    a_1@(3k+1) << 8; XOR63 a_1@2k | a_6@2k << 15."""
    fixed = np.asarray(fixed, dtype=np.uint32)
    a0, a1, a6, a9 = adv[0], adv[1], adv[6], adv[9]
    ones = np.uint64(M64)
    out = {}

    def u(col, rows):
        return col[rows].astype(np.uint64)

    for kind in ("add3", "add2"):
        r = _starts(fixed, kind)
        w = _word([u(a1, r + k) for k in range(4)])
        c = a9[r]
        out[kind + "_zero_c1"] = r[(w == 0) & (c == 1)]
        if kind == "add3":
            out["add3_zero_c2"] = r[(w == 0) & (c == 2)]
        out[kind + "_ones"] = r[w == ones]
    r = _starts(fixed, "xor")
    w = _word([u(a1, r + 2 * k) for k in range(4)])
    out["xor_zero"], out["xor_ones"] = r[w == 0], r[w == ones]
    r = _starts(fixed, "xor24")
    lo = [u(a1, r + 3 * k) for k in range(4)]
    hi = [u(a1, r + 3 * k + 1) for k in range(4)]
    w = _word([lo[k] | (hi[k] << np.uint64(8)) for k in range(4)])
    out["xor24_zero"], out["xor24_ones"] = r[w == 0], r[w == ones]
    edge = np.zeros(len(r), dtype=bool)
    for k in range(4):
        for j in (0, 1):
            edge |= (a1[r + 3 * k + j] == 0xff) & (a0[r + 3 * k + j] == 0)
    out["xor24_ff_tag0"] = r[edge]
    r = _starts(fixed, "xor63")
    w = _word([u(a1, r + 2 * k) | (u(a6, r + 2 * k) << np.uint64(15)) for k in range(4)])
    out["xor63_zero"], out["xor63_ones"] = r[w == 0], r[w == ones]
    edge = np.zeros(len(r), dtype=bool)
    for k in range(4):
        edge |= (a6[r + 2 * k] == 1) & (a1[r + 2 * k] == 0x7fff)
    out["xor63_zb1_7fff"] = r[edge]
    assert sorted(out) == sorted(CLASSES)
    return out


def expected_census(inputs):
    """{class: count} over the batch `inputs`, from g_trace alone (the init region's three XOR
    blocks included)."""
    n = dict.fromkeys(CLASSES, 0)

    def limbs(w):
        return [(w >> (16 * k)) & 0xffff for k in range(4)]

    for x in inputs:
        init, halves, _ = g_trace(int(x["rounds"]), x["h"], x["m"], x["t"], int(x["f"]))
        for w in init:
            n["xor_zero"] += w == 0
            n["xor_ones"] += w == M64
        for _, _, half, s3, xd, s2, xb in halves:
            n["add3_zero_c1"] += s3 == 1 << 64
            n["add3_zero_c2"] += s3 == 2 << 64
            n["add3_ones"] += s3 & M64 == M64
            n["add2_zero_c1"] += s2 == 1 << 64
            n["add2_ones"] += s2 & M64 == M64
            n["xor_zero"] += xd == 0
            n["xor_ones"] += xd == M64
            kind = "xor63" if half else "xor24"
            n[kind + "_zero"] += xb == 0
            n[kind + "_ones"] += xb == M64
            if half:
                n["xor63_zb1_7fff"] += any(v == 0xffff for v in limbs(xb))
            else:
                n["xor24_ff_tag0"] += any(v & 0xff == 0xff or v >> 8 == 0xff for v in limbs(xb))
    return n


# ------------------------------------------------------------------------------ the reference
class Reference:
    """The oracle's trace of batch(), its clean report and its census, computed once and left
    unchanged (the fault helpers flip a cell and flip it back)."""

    def __init__(self):
        import oracle

        oracle.lib()
        self.orc = oracle
        self.inputs = batch()
        self.n = len(self.inputs)
        self.used = int(oracle.offsets(self.inputs)[-1])
        self.total = self.used + PAD_ROWS
        self.adv, self.fixed, self.h_out, off = oracle.fill(self.inputs, total_rows=self.total)
        self.off = off.astype(np.uint64)
        self.clean = oracle.evaluate(self.adv, self.fixed, self.off)
        self.census = census(self.adv, self.fixed)
        self.h_ref = np.array([f_ref(int(x["rounds"]), x["h"], x["m"], x["t"], int(x["f"]))
                               for x in self.inputs], dtype=np.uint64)

    def instance_of(self, row):
        return min(int(np.searchsorted(self.off, row, side="right")) - 1, self.n - 1)

    def window(self, row):
        """(r0, r1, offsets re-based to r0) of the instances around `row` (one neighbour each
        side, as verdict_util.oracle_window takes them)."""
        i = self.instance_of(row)
        lo, hi = max(0, i - 1), min(self.n, i + 2)
        r0 = int(self.off[lo])
        r1 = self.total if hi == self.n else int(self.off[hi])  # the zero rows past the batch too
        return r0, r1, self.off[lo:hi + 1] - np.uint64(r0)

    def verdict(self, col, row, mask):
        """The oracle's report on the clean trace with `mask` XORed into cell (col, row) (col 10:
        the fixed column), evaluated on the window around the fault -- every other instance is
        clean -- and re-based: first_failure to the global row, rows_checked the batch's."""
        cell = self.fixed[row:row + 1] if col == 10 else self.adv[col, row:row + 1]
        r0, r1, sub = self.window(row)
        cell ^= np.uint32(mask)
        try:
            o = self.orc.evaluate(self.adv[:, r0:r1], self.fixed[r0:r1], sub, nthreads=1)
        finally:
            cell ^= np.uint32(mask)
        if o["first_failure"] != M64:
            o["first_failure"] += r0 << 8
        o["rows_checked"] = self.total
        return o


_reference = None


def reference():
    global _reference
    if _reference is None:
        _reference = Reference()
    return _reference


BLOCKS_PER_CLASS = 4


def faults(census_rows, adv):
    """[(class, col, row, mask)]: for up to BLOCKS_PER_CLASS blocks of every class (spread over the
    class's rows, the first and the last among them), bit 0 of one result limb's dense cell (a_1)
    and of one operand limb (a_3), the limb moving with the block; for ADD blocks, whose first row
    holds a carry in a_9 (the XOR blocks have no carry cell: a_9 is free there), bit 0 of the carry
    and, where the carry is 2, bit 1 as well."""
    out = []
    for cls in CLASSES:
        rows = census_rows[cls]
        pick = sorted({int(rows[(len(rows) - 1) * j // max(BLOCKS_PER_CLASS - 1, 1)])
                       for j in range(BLOCKS_PER_CLASS)}) if len(rows) else []
        stride, has_carry = CLASS_SHAPE[cls]
        for j, r in enumerate(pick):
            k = j % 4
            if has_carry:
                out.append((cls, 9, r, 1))
                if int(adv[9, r]) == 2:
                    out.append((cls, 9, r, 2))
            out.append((cls, 1, r + stride * k, 1))
            out.append((cls, 3, r + stride * ((k + 1) % 4), 1))
    return out
