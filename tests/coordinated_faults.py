"""Constraint-consistent multi-cell faults: the builder shared by tests/test_coordinated_faults_ref.py
(CPU) and tests/test_gpu_coordinated_faults.py (the product eval and the exact kernel).

A single-bit fault (tests/cell_sweep.py) almost always breaks several constraint families at once,
so that sweep never shows that one family is sound on its own. A fault here is a short list of
(col, row, value) writes to advice cells of one instance of a clean trace, built so that all
families but one still hold. It never touches the fixed column. L(x) = (tag(x), x, spread(x)); the
copy class of a cell is its equivalence class under the instance's copy constraints (union-find
over oracle.copies).

  L  lookup-consistent row substitution: (a_0, a_1, a_2) of a row become L(x'), x' = a_1 with one
     drawn bit below 16 flipped. Every lookup holds; gates and copies must see it. Every row, the
     zero rows past the instances included (there nothing constrains the row: accepted).
  C  copy-closed limb substitution: as L on a row whose a_1 or a_2 is in a copy class, and x' /
     spread(x') written to the whole class of a_1 / a_2 ("limb"); for a class whose source is an
     a_7 / a_8 cell (the XOR24 / XOR63 outputs) a new 16-bit value / its spread written to the whole
     class ("a7", "a8"). Every lookup and every copy holds: the gates alone must see it.
  S  gate-consistent operand shifts: every gate polynomial stays zero over Z, the copies alone must
     see it. "borrow": in an ADD block (gates 3, 5, 7, 9), operand column c, k = 0..2: c@k += 2^16,
     c@(k+1) -= 1. "carry": a_9@0 += 1, a_3@3 += 2^16 where the carry is below its maximum. "pair":
     at an operand row of an XOR-type gate (4, 6, 8, 10, 12, 13): a_3 += 1, a_4 -= 1 (gate 13 also
     (a_3, a_5) and (a_4, a_5)).
  W  zero mod 2^32, wrong over Z: at the same operand rows 2^31 XORed into a_3 and a_4. The gate
     must be counted; a checker that evaluates it in 32 bits sees the two copies only.
  T  range shifts that keep the XOR sum: XOR24, k with bit 0 of a_1@(3k+1) set: row 3k = L(lo |
     0x100), row 3k+1 = L(hi - 1); XOR63, k with a_6@2k = 1: row 2k = L(x | 0x8000), a_6@2k = 0. The
     sum polynomial stays zero and every lookup holds; the tag polynomials and the efgh / ijkl
     recompositions must see it.
  R  a range alone: class T's shifts are also seen by the 32-bit recompositions, so a checker whose
     tag and a_6 range terms checked nothing would still pass T. Here everything but the range holds
     mod 2^32 all the way down to the digest cells, on the blocks of G 4..7 of the last round (the
     last writers of v_4..v_7, whose XOR63 a_7 cells nobody copies). XOR63: "x15" (k < 3, a_6@2k =
     1): row 2k = L(x | 0x8000), a_6@2k = 0, a_7@2k += 2^16, a_7@(2k+2) -= 1 (the word unchanged
     over Z), a_8@2k left as it is (its polynomial is -2^32), a_8@(2k+2) -= 1; "a6" (bit 1 of limb
     k+1 clear): a_6@2k += 4 (2^30 a_6 becomes 2^32), a_7 and a_8 of row 2((k+1) & 3) += 4. The
     changed limb is carried through the final XOR3 block that copies it: its a_4, L(e), L(j) and
     the digest cell recomputed. XOR24: "hi8" (bit 8 of output limb k-1 clear): row 3k+1 = L(hi |
     0x100) (2^16 a_2@(3k+1) moves the sum by 2^32), the output limb gains bit 8; "lo8" (k != 1, bit
     0 of hi set): class T's rows with the recompositions followed: a_7 of limb k-2 += 2^16, of limb
     k-1 -= 1 (the same word over Z for the ADD3 that copies it), a_8 of limb k-2 left as it is
     (-2^32), of limb k-1 -= 1. Everything downstream of the new b is re-derived as the synthesis
     would (`_tail`: ADD3 a2, XOR d2, ADD2 c2, XOR63, four final XOR3 blocks); an R fault writes 7 to 80 cells.
     Every lookup, every copy and every other polynomial holds over Z; only the tag (x15, lo8: and
     one a_8 recomposition by 2^32; hi8: and the sum by 2^32) or a_6 (a_6 - 1) and the sum by 2^32
     (a6) do not.

Batch A (cell_sweep.batch("A")): every applicable site of every class. Batch B: the sites whose
written cells touch cell_sweep's windows, and in addition class C and the a_5 borrow of class S on
the message limbs of the 13-round instance (INW rows 32..95; the borrow in every round's ADD3
blocks, k = 0..2, which reaches every limb in every round): their copy classes have 14 cells
across every round and are the only route to the fast pass's message-copy compare.

A site where the shift cannot be made (a cell that would go below zero) is skipped and counted.
Drawn bits are indexed by the cell, not by the order of iteration.
"""
import numpy as np

import cell_sweep as cs
from verdict_util import INIT_ROWS, NONE, ROUND_ROWS

CLASSES = ("L", "C", "S", "W", "T", "R")
SEED = {"A": 7101, "B": 7102}  # this file's own draws (cell_sweep's seeds are not touched)
ADD_GATES = {3: (3, 4, 5), 5: (3, 4), 7: (3, 4, 5), 9: (3, 4)}  # selector bit -> operand columns
ADD_MAX_CARRY = {3: 2, 5: 1, 7: 2, 9: 1}
XOR_GATES = {4: 3, 6: 2, 8: 2, 10: 2, 12: 2, 13: 2}  # selector bit -> rows per limb
XOR_PAIRS = {13: ((3, 4), (3, 5), (4, 5))}  # the others: (a_3, a_4)
MSG_ROWS = (32, 96)  # INW rows of the message words, instance-relative

# Pinned by tests/test_coordinated_faults_ref.py and asserted again by the GPU test.
# per batch and class: (faults, sites, skipped sites, faults the oracle rejects)
COUNTS = {"A": {"L": (2584, 2584, 0, 2576), "C": (1776, 1776, 0, 1776), "S": (1975, 1983, 8, 1975),
                "W": (688, 688, 0, 688), "T": (123, 123, 0, 123), "R": (81, 81, 0, 81)},
          "B": {"L": (688, 688, 0, 688), "C": (800, 800, 0, 800), "S": (1232, 1232, 0, 1232),
                "W": (224, 224, 0, 224), "T": (46, 46, 0, 46), "R": (24, 24, 0, 24)}}
SHAPES = {"A": {("C", "limb"): 1312, ("C", "a7"): 208, ("C", "a8"): 256, ("S", "borrow"): 960,
                ("S", "carry"): 79, ("S", "pair"): 936, ("T", "xor24"): 65, ("T", "xor63"): 58,
                ("R", "x15"): 21, ("R", "a6"): 26, ("R", "hi8"): 18, ("R", "lo8"): 16},
          "B": {("C", "limb"): 528, ("C", "a7"): 128, ("C", "a8"): 144, ("S", "borrow"): 912,
                ("S", "carry"): 32, ("S", "pair"): 288, ("T", "xor24"): 23, ("T", "xor63"): 23,
                ("R", "x15"): 6, ("R", "a6"): 9, ("R", "hi8"): 5, ("R", "lo8"): 4}}


def tag(x):
    return 0 if x < 1 << 8 else 1 if x < 1 << 15 else 2


def spread(x):
    assert 0 <= x < 1 << 16
    s = 0
    for i in range(16):
        s |= ((x >> i) & 1) << (2 * i)
    return s


def unspread(s):
    assert s & 0xaaaaaaaa == 0
    return sum(((s >> (2 * i)) & 1) << i for i in range(16))


def L(x):
    return (tag(x), x, spread(x))


def is_table_row(t, d, s):
    """The lookup of docs/LAYOUT.md §3, in plain Python."""
    return 0 <= d < 1 << 16 and t == tag(d) and s == spread(d)


class Fault:
    __slots__ = ("cls", "shape", "gate", "row", "sub", "writes", "block")

    def __init__(self, cls, shape, gate, row, sub, writes, block=None):
        seen = {}
        for c, r, v in writes:
            assert 0 <= c < 10 and 0 <= v < 1 << 32
            assert seen.setdefault((c, r), v) == v, "two values for one cell"
        self.cls, self.shape, self.gate, self.row, self.sub = cls, shape, gate, int(row), sub
        self.writes = tuple((c, r, v) for (c, r), v in sorted(seen.items()))
        self.block = block  # first row of the gate's block, where the fault is tied to one

    @property
    def key(self):
        return (self.cls, self.shape, self.gate, self.row, self.sub)

    def __repr__(self):
        return "%s/%s gate %s row %d %s writes %s" % (
            self.cls, self.shape, self.gate, self.row, self.sub,
            ["a_%d[%d]=%#x" % w for w in self.writes])


_classes_of_rounds = {}


def copy_classes(rounds):
    """{(col, row): tuple of the cells of its copy class} of one instance of `rounds` rounds,
    instance-relative rows, for every cell that is in a copy constraint."""
    if rounds in _classes_of_rounds:
        return _classes_of_rounds[rounds]
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for dr, dc, sr, sc in cs._orc().copies(int(rounds)).astype(np.int64):
        a, b = find((int(dc), int(dr))), find((int(sc), int(sr)))
        if a != b:
            parent[a] = b
    groups = {}
    for x in parent:
        groups.setdefault(find(x), []).append(x)
    out = {}
    for g in groups.values():
        g = tuple(sorted(g))
        for x in g:
            out[x] = g
    _classes_of_rounds[rounds] = out
    return out


class Faults:
    """The faults of one batch: by_class[cls] the list (in site order), sites[cls] and
    skipped[cls] the counts of applicable and of skipped sites, stats the finer counts."""

    def __init__(self, name):
        self.name = name
        self.b = b = cs.batch(name)
        self.adv = b.adv
        self.sel = b.fixed & np.uint32(0xffff)
        rng = np.random.default_rng(SEED[name])
        self.bit = rng.integers(0, 16, (4, b.total))  # per row: L, C limb, C a7, C a8
        self.window = None if name == "A" else set(int(r) for r in b.rows)
        self.by_class = {c: [] for c in CLASSES}
        self.sites = {c: 0 for c in CLASSES}
        self.skipped = {c: 0 for c in CLASSES}
        self.stats = {"add_blocks": 0, "carry": {g: 0 for g in ADD_GATES}, "t_sites": 0,
                      "c_rows": 0, "c_a78": 0, "msg_c": 0, "msg_borrow": 0, "r_sites": 0}
        self._build()

    # ------------------------------------------------------------------ helpers
    def _a(self, c, r):
        return int(self.adv[c, r])

    def _blocks(self, gate):
        return [int(r) for r in np.flatnonzero((self.sel >> np.uint32(gate)) & np.uint32(1))]

    def _wanted(self, writes, extra=False):
        return extra or self.window is None or any(r in self.window for _, r, _ in writes)

    def _add(self, fault, extra=False):
        """Count the site; keep it if it is in the batch's scope. Returns whether it was kept."""
        if not self._wanted(fault.writes, extra):
            return False
        self.sites[fault.cls] += 1
        self.by_class[fault.cls].append(fault)
        return True

    def _skip(self, cls, cells, extra=False):
        if self._wanted([(c, r, 0) for c, r in cells], extra):
            self.sites[cls] += 1
            self.skipped[cls] += 1

    def _row_sub(self, r, which):
        x = self._a(1, r) ^ (1 << int(self.bit[which, r]))
        return x, [(0, r, tag(x)), (1, r, x), (2, r, spread(x))]

    # ------------------------------------------------------------------ the classes
    def _build(self):
        b = self.b
        for r in range(b.total):  # L
            _, w = self._row_sub(r, 0)
            self._add(Fault("L", "row", None, r, None, w))
        for i, rounds in enumerate(b.rounds):  # C
            base, end = int(b.off[i]), int(b.off[i + 1])
            cl = copy_classes(int(rounds))
            msg = self.name == "B" and i == 1
            for r in range(base, end):
                c1, c2 = cl.get((1, r - base)), cl.get((2, r - base))
                if c1 is None and c2 is None:
                    continue
                x, w = self._row_sub(r, 1)
                w += [(c, base + rr, x) for c, rr in (c1 or ())]
                w += [(c, base + rr, spread(x)) for c, rr in (c2 or ())]
                extra = msg and MSG_ROWS[0] <= r - base < MSG_ROWS[1]
                if self._add(Fault("C", "limb", None, r, None, w), extra):
                    self.stats["c_rows"] += 1
                    self.stats["msg_c"] += extra
            for col, which in ((7, 2), (8, 3)):
                for r in range(base, end):
                    g = cl.get((col, r - base))
                    if g is None:
                        continue
                    assert [c for c, _ in g if c not in (3, 4, 5)] == [col]  # the class's one source
                    v = self._a(7, r) ^ (1 << int(self.bit[which, r]))
                    assert self._a(8, r) == spread(self._a(7, r))
                    v = v if col == 7 else spread(v)
                    w = [(c, base + rr, v) for c, rr in g]
                    if self._add(Fault("C", "a%d" % col, None, r, None, w)):
                        self.stats["c_a78"] += 1
        msg_lo = int(b.off[1]) if self.name == "B" else None
        msg_hi = int(b.off[2]) if self.name == "B" else None
        for gate, cols in ADD_GATES.items():  # S: borrow and carry
            for r0 in self._blocks(gate):
                for col in cols:
                    for k in range(3):
                        extra = col == 5 and msg_lo is not None and msg_lo <= r0 < msg_hi
                        lo, hi = self._a(col, r0 + k), self._a(col, r0 + k + 1)
                        if hi == 0:
                            self._skip("S", [(col, r0 + k), (col, r0 + k + 1)], extra)
                            continue
                        w = [(col, r0 + k, lo + (1 << 16)), (col, r0 + k + 1, hi - 1)]
                        if self._add(Fault("S", "borrow", gate, r0 + k, "a_%d" % col, w, r0), extra):
                            self.stats["msg_borrow"] += extra
        for gate in ADD_GATES:
            for r0 in self._blocks(gate):
                w = [(9, r0, self._a(9, r0) + 1), (3, r0 + 3, self._a(3, r0 + 3) + (1 << 16))]
                if not self._wanted(w):
                    continue
                self.stats["add_blocks"] += 1
                if self._a(9, r0) < ADD_MAX_CARRY[gate]:
                    self._add(Fault("S", "carry", gate, r0, None, w, r0))
                    self.stats["carry"][gate] += 1
        for gate, step in XOR_GATES.items():  # S: pair, and W
            for r0 in self._blocks(gate):
                for k in range(4):
                    r = r0 + step * k
                    for up, down in XOR_PAIRS.get(gate, ((3, 4),)):
                        u, d = self._a(up, r), self._a(down, r)
                        if d == 0:
                            self._skip("S", [(up, r), (down, r)])
                            continue
                        self._add(Fault("S", "pair", gate, r, "a_%d,a_%d" % (up, down),
                                        [(up, r, u + 1), (down, r, d - 1)], r0))
                    self._add(Fault("W", "top", gate, r, None,
                                    [(3, r, self._a(3, r) ^ (1 << 31)), (4, r, self._a(4, r) ^ (1 << 31))], r0))
        for r0 in self._blocks(4):  # T, XOR24
            for k in range(4):
                lo, hi = self._a(1, r0 + 3 * k), self._a(1, r0 + 3 * k + 1)
                assert lo < 256 and hi < 256
                cells = [(c, r0 + 3 * k + j) for j in (0, 1) for c in (0, 1, 2)]
                if not self._wanted([(c, r, 0) for c, r in cells]):
                    continue
                self.stats["t_sites"] += 1
                if hi & 1:
                    w = [(c, r0 + 3 * k, v) for c, v in enumerate(L(lo | 0x100))]
                    w += [(c, r0 + 3 * k + 1, v) for c, v in enumerate(L(hi - 1))]
                    self._add(Fault("T", "xor24", 4, r0 + 3 * k, None, w, r0))
        for r0 in self._blocks(8):  # T, XOR63
            for k in range(4):
                r = r0 + 2 * k
                x, z = self._a(1, r), self._a(6, r)
                assert x < 1 << 15 and z < 2
                cells = [(0, r), (1, r), (2, r), (6, r)]
                if not self._wanted([(c, rr, 0) for c, rr in cells]):
                    continue
                self.stats["t_sites"] += 1
                if z == 1:
                    w = [(c, r, v) for c, v in enumerate(L(x | 0x8000))] + [(6, r, 0)]
                    self._add(Fault("T", "xor63", 8, r, None, w, r0))
        for i, rounds in enumerate(b.rounds):  # R: the last XOR63 of v_4..v_7 (G 4..7 of the last round)
            if rounds == 0:
                continue
            base = int(b.off[i])
            cl = copy_classes(int(rounds))
            for g in range(4, 8):
                # docs/LAYOUT.md §5: G g of the last round at 164 + 416 (rounds - 1) + 52 g, its XOR63 at +44
                r0 = base + INIT_ROWS + ROUND_ROWS * (int(rounds) - 1) + 52 * g + 44
                assert int(self.sel[r0]) == (1 << 8) | (1 << 2)
                for k in range(4):
                    r, k1 = r0 + 2 * k, (k + 1) & 3
                    r1 = r0 + 2 * k1
                    x, z, w1 = self._a(1, r), self._a(6, r), self._a(7, r1)
                    assert cl.get((7, r1 - base)) is None and self._a(8, r1) == spread(w1) and (w1 & 1) == z
                    # x15: a_1@2k takes the top bit a_6@2k held; word b stays the same over Z (k < 3)
                    if k < 3:
                        w = [(c, r, v) for c, v in enumerate(L(x | 0x8000))]
                        w += [(6, r, 0), (7, r, self._a(7, r) + (1 << 16)), (7, r1, w1 - z)]
                        w += self._final_limb(base, cl, r1, k1, w1 & ~1)
                        if self._wanted(w):
                            self.stats["r_sites"] += 1
                            if z == 1:
                                self._add(Fault("R", "x15", 8, r, None, self._changed(w), r0))
                    # a6: a_6@2k += 4, which 2^30 a_6 turns into 2^32
                    w = [(6, r, z + 4), (7, r1, w1 + 4)] + self._final_limb(base, cl, r1, k1, w1 | 2)
                    if self._wanted(w):
                        self.stats["r_sites"] += 1
                        if not w1 & 2:
                            self._add(Fault("R", "a6", 8, r, None, self._changed(w), r0))
                # the XOR24 of the same G: its output b feeds ADD3 a2 (dense) and this XOR63 (spread)
                r0 = base + INIT_ROWS + ROUND_ROWS * (int(rounds) - 1) + 52 * g + 16  # §5: XOR24 at +16
                assert int(self.sel[r0]) == (1 << 4) | (1 << 1)
                bw = [self._a(7, r0 + 3 * q) for q in range(4)]
                assert not self._changed(self._tail(base, int(rounds), g, bw, bw)), "the model is not the trace"
                for k in range(4):
                    lo, hi = self._a(1, r0 + 3 * k), self._a(1, r0 + 3 * k + 1)
                    j2, j1 = (k + 2) & 3, (k + 3) & 3  # a_7@3j2 reads 2^8 lo_k, a_7@3j1 reads hi_k
                    # hi8: a_1@(3k+1) += 2^8, which 2^16 a_2@(3k+1) turns into 2^32; limb j1 of b gains bit 8
                    bd = list(bw)
                    bd[j1] |= 0x100
                    w = [(c, r0 + 3 * k + 1, v) for c, v in enumerate(L(hi | 0x100))]
                    w += [(7, r0 + 3 * j1, bd[j1]), (8, r0 + 3 * j1, spread(bd[j1]))]
                    w += self._tail(base, int(rounds), g, bd, bd)
                    if self._wanted(w):
                        self.stats["r_sites"] += 1
                        if not bw[j1] & 0x100:
                            self._add(Fault("R", "hi8", 4, r0 + 3 * k + 1, None, self._changed(w), r0))
                    # lo8: class T's shift with the recompositions followed: b is the same word over Z for
                    # the ADD3 (limb j2 += 2^16, limb j1 -= 1; k != 1), the XOR63 sees bit 0 of limb j1 cleared
                    if k != 1:
                        bd, bs = list(bw), list(bw)
                        bd[j2] += 1 << 16
                        bd[j1] -= hi & 1
                        bs[j1] &= ~1
                        w = [(c, r0 + 3 * k, v) for c, v in enumerate(L(lo | 0x100))]
                        w += [(c, r0 + 3 * k + 1, v) for c, v in enumerate(L(hi & ~1))]
                        w += [(7, r0 + 3 * j2, bd[j2]), (7, r0 + 3 * j1, bd[j1]), (8, r0 + 3 * j1, spread(bs[j1]))]
                        w += self._tail(base, int(rounds), g, bd, bs)
                        if self._wanted(w):
                            self.stats["r_sites"] += 1
                            if hi & 1:
                                self._add(Fault("R", "lo8", 4, r0 + 3 * k, None, self._changed(w), r0))

    def _changed(self, writes):
        return [(c, r, v) for c, r, v in writes if self._a(c, r) != v]

    def _limbs(self, col, r0, step=1, f=int):
        return [f(self._a(col, r0 + step * q)) for q in range(4)]

    def _tail(self, base, rounds, g, bd, bs):
        """Every cell downstream of word b = the XOR24 output of G g (4..7) of the last round,
        re-derived as the synthesis of docs/LAYOUT.md §5 would from new limbs of b: `bd` as the ADD3
        a2 copies them (dense; a limb may exceed 16 bits) and `bs` as the XOR63 copies them
        (spread(bs[q])). The other operands are read from the blocks' own operand cells. ADD3 a2,
        XOR d2, ADD2 c2, XOR63, then the final XOR3 blocks of the G's four words."""
        # docs/LAYOUT.md §5: G g of round r starts at 164 + 416 r + 52 g and holds ADD3 a1 at +0, XOR d1
        # at +4, ADD2 c1 at +12, XOR24 at +16, ADD3 a2 at +28, XOR d2 at +32, ADD2 c2 at +40, XOR63 at
        # +44; the final XOR3 block of h'_i (H = h_i, V = v_i, U = v_{i+8}) is at 164 + 416 rounds + 8 i;
        # (a, b, c, d) of G 4..7 are the diagonals of the §5 table
        gb = base + INIT_ROWS + ROUND_ROWS * (rounds - 1) + 52 * g
        fb = base + INIT_ROWS + ROUND_ROWS * rounds
        ia, ib, ic, id_ = ((0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))[g - 4]
        val = lambda l: sum(v << (16 * q) for q, v in enumerate(l))  # noqa: E731
        split = lambda x: [(x >> (16 * q)) & 0xffff for q in range(4)]  # noqa: E731
        rows = lambda r0, step, l: [(c, r0 + step * q, v) for q in range(4) for c, v in enumerate(L(l[q]))]  # noqa: E731
        w = []
        r0 = gb + 28  # ADD3 a2 = a + b + y
        tot = val(self._limbs(3, r0)) + val(bd) + val(self._limbs(5, r0))
        a2 = split(tot)
        w += [(4, r0 + q, bd[q]) for q in range(4)] + rows(r0, 1, a2) + [(9, r0, tot >> 64)]
        r0 = gb + 32  # XOR d2 = (d ^ a2) >>> 16
        x = self._limbs(3, r0, 2, unspread)
        w += [(4, r0 + 2 * q, spread(a2[q])) for q in range(4)]
        z = [x[q] ^ a2[q] for q in range(4)]
        w += rows(r0, 2, z) + rows(r0 + 1, 2, [x[q] & a2[q] for q in range(4)])
        d2 = [z[(q + 1) & 3] for q in range(4)]
        r0 = gb + 40  # ADD2 c2 = c + d2
        tot = val(self._limbs(3, r0)) + val(d2)
        c2 = split(tot)
        w += [(4, r0 + q, d2[q]) for q in range(4)] + rows(r0, 1, c2) + [(9, r0, tot >> 64)]
        r0 = gb + 44  # XOR63 b2 = (b ^ c2) >>> 63
        w += [(3, r0 + 2 * q, spread(bs[q])) for q in range(4)] + [(4, r0 + 2 * q, spread(c2[q])) for q in range(4)]
        zw = val(bs) ^ val(c2)
        z = split(zw)
        w += rows(r0, 2, [v & 0x7fff for v in z]) + rows(r0 + 1, 2, [bs[q] & c2[q] for q in range(4)])
        b2 = split(((zw << 1) | (zw >> 63)) & (2**64 - 1))
        for q in range(4):
            w += [(6, r0 + 2 * q, z[q] >> 15), (7, r0 + 2 * q, b2[q]), (8, r0 + 2 * q, spread(b2[q]))]
        for i, col, word in ((ia, 4, a2), (ib, 4, b2), (ic - 8, 5, c2), (id_ - 8, 5, d2)):  # final XOR3
            r0 = fb + 8 * i
            assert int(self.sel[r0]) == (1 << 13) | (1 << 11)
            op = {c: self._limbs(c, r0, 2, unspread) for c in (3, 4, 5)}
            op[col] = word  # the four words of a G meet four different blocks
            h, v, u = op[3], op[4], op[5]
            e = [h[q] ^ v[q] ^ u[q] for q in range(4)]
            w += [(col, r0 + 2 * q, spread(word[q])) for q in range(4)] + rows(r0, 2, e)
            w += rows(r0 + 1, 2, [(h[q] & v[q]) | (h[q] & u[q]) | (v[q] & u[q]) for q in range(4)])
            w += [(7, r0, e[0] | e[1] << 16), (8, r0, e[2] | e[3] << 16)]
        return w

    def _final_limb(self, base, cl, r1, k1, v):
        """The writes that make limb k1 of the word whose canonical spread cell is a_8[r1] read `v`
        downstream: a_8[r1] and its copy (a_4 of the final XOR3 block of that word), that row
        pair's L(e), L(j) recomputed, and the digest cell that recomposes e."""
        g = cl[(8, r1 - base)]
        (dest,) = [(c, rr) for c, rr in g if c != 8]
        assert dest[0] == 4
        rf = base + dest[1]
        fb = rf - 2 * k1
        assert int(self.sel[fb]) == (1 << 13) | (1 << 11)
        h, u = unspread(self._a(3, rf)), unspread(self._a(5, rf))
        assert unspread(self._a(4, rf)) == self._a(7, r1) and self._a(1, rf) == h ^ self._a(7, r1) ^ u
        e, j = h ^ v ^ u, (h & v) | (h & u) | (v & u)
        w = [(8, r1, spread(v)), (4, rf, spread(v))]
        w += [(c, rf, x) for c, x in enumerate(L(e))] + [(c, rf + 1, x) for c, x in enumerate(L(j))]
        lo = [e if 2 * q == 2 * k1 else self._a(1, fb + 2 * q) for q in range(4)]
        w.append((7, fb, lo[0] | lo[1] << 16) if k1 < 2 else (8, fb, lo[2] | lo[3] << 16))
        return w

    # ------------------------------------------------------------------ views
    def all(self):
        return [f for c in CLASSES for f in self.by_class[c]]

    def n_rejected(self, cls):
        return sum(1 for f in self.by_class[cls] if rejected(verdict(self.name, f)))


_faults = {}
_verdicts = {}


def faults(name):
    if name not in _faults:
        _faults[name] = Faults(name)
    return _faults[name]


def applied(name, fault):
    """Context manager: the batch's host trace with the fault written, restored on exit."""
    return _Applied(cs.batch(name).adv, fault)


class _Applied:
    def __init__(self, adv, fault):
        self.adv, self.fault = adv, fault

    def __enter__(self):
        self.old = [int(self.adv[c, r]) for c, r, _ in self.fault.writes]
        for c, r, v in self.fault.writes:
            self.adv[c, r] = v
        return self.adv

    def __exit__(self, *exc):
        for (c, r, _), v in zip(self.fault.writes, self.old):
            self.adv[c, r] = v
        return False


def verdict(name, fault):
    """The oracle's report on the batch's clean trace with the fault written, memoised: the GPU
    checkers share one CPU evaluation per fault. Batch B as cell_sweep.oracle_verdict does it: the
    oracle runs on the instances around the fault (a fault lies within one instance)."""
    key = (name,) + fault.key
    if key in _verdicts:
        return _verdicts[key]
    orc = cs._orc()
    b = cs.batch(name)
    inst = {b.instance_of(r) for _, r, _ in fault.writes}
    assert len(inst) == 1, fault
    with applied(name, fault):
        if name == "A":
            o = orc.evaluate(b.adv, b.fixed, b.off, nthreads=1)
        else:
            i = inst.pop()
            lo, hi = max(0, i - 1), min(b.n, i + 2)
            r0 = int(b.off[lo])
            r1 = b.total if hi == b.n else int(b.off[hi])
            o = orc.evaluate(b.adv[:, r0:r1], b.fixed[r0:r1], b.off[lo:hi + 1] - np.uint64(r0), nthreads=1)
            if o["first_failure"] != NONE:
                o["first_failure"] += r0 << 8
            o["rows_checked"] = b.total
    _verdicts[key] = o
    return o


def rejected(report):
    return report["first_failure"] != NONE


assert INIT_ROWS == 164 and ROUND_ROWS == 416
