"""tests/coordinated_faults.py pinned on the CPU, so the GPU test cannot pass on mislabelled faults.

For every fault of every class on both batches: the rows it writes in a_0..a_2 hold table rows
(checked in plain Python, not through the oracle); class C leaves every copy constraint equal;
classes S and T leave the named polynomials of tests/quotient_gates_ref.py zero over Python
integers on the block; class W moves the named polynomial by exactly 2^32 (non-zero over Z, zero mod
2^32); and the oracle's report has the signature the constraint system predicts for the class:

  L  lookup_failures unchanged; every instance row rejected, the zero rows past the instances
     accepted with the clean report; on batch A 1,264 of the 2,576 rejected with no copy failure.
  C  rejected by gates alone: copy_failures = lookup_failures = 0.
  S  no gate counter moves; copy_failures = 2 (borrow, pair) or 1 (carry), reported at the first
     written operand cell.
  W  the gate's counter is 1, no other gate moves; copy_failures = 2.
  T  lookup_failures = copy_failures = 0; the block's sum gate (4 / 8) counted for its tag and the
     recomposition gate (1 / 2) for the moved limb, no other.
  R  lookup_failures = copy_failures = 0; x15: gate 8 for the tag and gate 2 for one a_8 polynomial
     (exactly -2^32); a6: gate 8 alone, its sum polynomial exactly -2^32 and a_6 (a_6 - 1) non-zero;
     hi8: gate 4 alone, its sum polynomial exactly -2^32 and the tag; lo8: gate 4 for the tag and
     gate 1 for one a_8 polynomial (exactly -2^32). Every other polynomial of the G's blocks from
     the XOR24 on and of the eight final XOR3 blocks is zero over Python integers.

The case counts are pinned per class and batch, with the caps that keep a class from hollowing out:
skipped sites at most 5 % of a class's sites, the carry raise on at least half of the ADD blocks and
under each of the four ADD selectors, T and R on at least a quarter of their k-sites. The counts are printed
(`-s`): tests/test_gpu_coordinated_faults.py asserts the same numbers."""
import numpy as np
import pytest

import cell_sweep as cs
import coordinated_faults as cf
import quotient_gates_ref as gr

COUNTS, SHAPES = cf.COUNTS, cf.SHAPES


def _copies(b):
    """(dst col, dst row, src col, src row) index arrays of every copy constraint of the batch."""
    out = []
    for i, r in enumerate(b.rounds):
        q = cs._orc().copies(int(r)).astype(np.int64)
        base = int(b.off[i])
        out.append(np.stack([q[:, 1], q[:, 0] + base, q[:, 3], q[:, 2] + base]))
    return np.concatenate(out, axis=1)


def _polys(adv, gate, r0):
    return gr.GATES[gate](lambda c, j: int(adv[c, r0 + j]))


def _sum_index(gate, k):
    return 3 * k if gate in (4, 8) else k


def _gates(o):
    return {g: int(v) for g, v in enumerate(o["gate_failures"]) if v}


def _check_range(b, f, adv):
    """Class R on the faulted trace: the block's own polynomials are what the shape says, and every
    block downstream (the rest of the G, the eight final XOR3 blocks) is zero over Z."""
    inst = b.instance_of(f.row)
    base, rounds = int(b.off[inst]), int(b.rounds[inst])
    gb = f.block - (44 if f.gate == 8 else 16)
    assert (gb - base - 164 - 416 * (rounds - 1)) % 52 == 0 and 4 <= (gb - base - 164 - 416 * (rounds - 1)) // 52 < 8
    want = {g: [0] * gr.GATE_COUNTS[g] for g in (1, 2, 4, 8)}
    if f.shape == "x15":
        k = (f.row - f.block) // 2
        assert int(adv[0, f.row]) == 2
        want[8][3 * k + 1] = 2
        want[2][2 * k + 1] = -(1 << 32)
    elif f.shape == "a6":
        k = (f.row - f.block) // 2
        z = int(adv[6, f.row])
        assert z in (4, 5)
        want[8][3 * k], want[8][3 * k + 2] = -(1 << 32), z * (z - 1)
    elif f.shape == "hi8":
        k = (f.row - f.block) // 3
        want[4][3 * k], want[4][3 * k + 2] = -(1 << 32), 1
    else:
        k = (f.row - f.block) // 3
        want[4][3 * k + 1] = 1
        want[1][2 * ((k + 2) & 3) + 1] = -(1 << 32)
    for g, r0 in ((4, gb + 16), (1, gb + 16), (7, gb + 28), (10, gb + 32), (9, gb + 40), (8, gb + 44), (2, gb + 44)):
        assert (int(b.fixed[r0]) >> g) & 1
        assert _polys(adv, g, r0) == want.get(g, [0] * gr.GATE_COUNTS[g]), (f, g)
    fb = base + 164 + 416 * rounds
    for i in range(8):
        assert int(b.fixed[fb + 8 * i]) & 0xffff == (1 << 13) | (1 << 11)
        assert not any(_polys(adv, 13, fb + 8 * i)) and not any(_polys(adv, 11, fb + 8 * i)), f
    assert any(r >= fb for _, r, _ in f.writes), "the fault does not reach the final blocks"


def _check(name, b, f, cp):
    clean = b.clean
    with cf.applied(name, f) as adv:
        for r in {r for c, r, _ in f.writes if c < 3}:
            assert cf.is_table_row(int(adv[0, r]), int(adv[1, r]), int(adv[2, r])), f
        if f.cls in ("C", "R"):
            assert np.array_equal(adv[cp[0], cp[1]], adv[cp[2], cp[3]]), f
        if f.cls == "S":  # every polynomial of the gate zero over Z on the block
            assert not any(_polys(adv, f.gate, f.block)), f
        if f.cls == "T":  # the four sum polynomials zero over Z; a tag polynomial is what fails
            p = _polys(adv, f.gate, f.block)
            k = (f.row - f.block) // cf.XOR_GATES[f.gate]
            assert not any(p[_sum_index(f.gate, q)] for q in range(4)), f
            assert p[3 * k + 1] == (1 if f.shape == "xor24" else 2), f
            assert not any(v for i, v in enumerate(p) if i != 3 * k + 1), f
        if f.cls == "W":  # the limb's sum polynomial exactly 2^32: non-zero over Z, zero mod 2^32
            k = (f.row - f.block) // cf.XOR_GATES[f.gate]
            p = _polys(adv, f.gate, f.block)
            assert p[_sum_index(f.gate, k)] == 1 << 32 and p[_sum_index(f.gate, k)] % (1 << 32) == 0, f
            assert not any(v for i, v in enumerate(p) if i != _sum_index(f.gate, k)), f
        if f.cls == "R":
            _check_range(b, f, adv)
    o = cf.verdict(name, f)
    assert o["rows_checked"] == b.total and o["fixed_failures"] == 0, f
    assert o["lookup_failures"] == clean["lookup_failures"] == 0, f
    if f.cls == "L":
        if f.row < b.used:
            assert cf.rejected(o) and (_gates(o) or o["copy_failures"]), f
        else:
            assert o == clean, f
    elif f.cls == "C":
        assert cf.rejected(o) and o["copy_failures"] == 0 and _gates(o), f
    elif f.cls == "S":
        dests = sorted(r for c, r, _ in f.writes if c != 9)
        assert not _gates(o) and o["copy_failures"] == len(dests) == (1 if f.shape == "carry" else 2), f
        assert o["first_failure"] == (dests[0] << 8) | 17, f
    elif f.cls == "W":
        assert _gates(o) == {f.gate: 1} and o["copy_failures"] == 2, f
        assert o["first_failure"] == (f.block << 8) | f.gate, f
    elif f.cls == "T":
        assert _gates(o) == ({1: 1, 4: 1} if f.shape == "xor24" else {2: 1, 8: 1}), f
        assert o["copy_failures"] == 0 and cf.rejected(o), f
    else:
        want = {"x15": {2: 1, 8: 1}, "a6": {8: 1}, "hi8": {4: 1}, "lo8": {1: 1, 4: 1}}[f.shape]
        assert _gates(o) == want and o["copy_failures"] == 0, f
        assert o["first_failure"] == (f.block << 8) | min(want), f


@pytest.mark.parametrize("cls", cf.CLASSES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_fault_is_what_its_class_says(orc, name, cls):
    b = cs.batch(name)
    fs = cf.faults(name)
    cp = _copies(b)
    assert np.array_equal(b.adv[cp[0], cp[1]], b.adv[cp[2], cp[3]])
    before = b.adv.copy()
    for f in fs.by_class[cls]:
        assert f.cls == cls
        _check(name, b, f, cp)
    assert np.array_equal(b.adv, before), "a fault was not undone"
    got = (len(fs.by_class[cls]), fs.sites[cls], fs.skipped[cls], fs.n_rejected(cls))
    print("batch %s class %s: %d faults, %d sites, %d skipped, %d rejected" % ((name, cls) + got))
    assert got == COUNTS[name][cls]
    assert fs.sites[cls] == len(fs.by_class[cls]) + fs.skipped[cls]
    assert fs.skipped[cls] * 20 <= fs.sites[cls], "more than 5 % of the class's sites skipped"


@pytest.mark.parametrize("name", ["A", "B"])
def test_counts_and_caps(orc, name):
    b = cs.batch(name)
    fs = cf.faults(name)
    keys = [f.key for f in fs.all()]
    assert len(set(keys)) == len(keys)
    shapes = {}
    for f in fs.all():
        shapes[(f.cls, f.shape)] = shapes.get((f.cls, f.shape), 0) + 1
        assert len({b.instance_of(r) for _, r, _ in f.writes}) == 1
        assert 2 <= len(f.writes) <= (17 if f.cls != "R" else 80), f
        assert all(int(b.adv[c, r]) != v for c, r, v in f.writes if f.cls != "L" and c != 0), f
    for k, n in SHAPES[name].items():
        assert shapes.get(k) == n, (k, shapes.get(k))
    st = fs.stats
    print("batch %s: %s, carry raise on %d of %d ADD blocks %r, T on %d of %d k-sites"
          % (name, shapes, sum(st["carry"].values()), st["add_blocks"], st["carry"],
             len(fs.by_class["T"]), st["t_sites"]))
    assert 2 * sum(st["carry"].values()) >= st["add_blocks"] and all(st["carry"].values())
    assert 4 * len(fs.by_class["T"]) >= st["t_sites"]
    assert 4 * len(fs.by_class["R"]) >= st["r_sites"] == (168 if name == "A" else 56)
    assert st["c_rows"] == SHAPES[name][("C", "limb")]
    if name == "A":
        classes = sum(len(set(cf.copy_classes(int(r)).values())) for r in b.rounds)
        sizes = {len(g) for r in b.rounds for g in cf.copy_classes(int(r)).values()}
        assert classes == 2544 and sizes == {2, 3}
        assert (st["add_blocks"], sum(st["carry"].values()), st["t_sites"]) == (128, 79, 256)
        # the rejected faults of L that no copy sees: gates alone
        gates_only = sum(1 for f in fs.by_class["L"]
                         if cf.rejected(cf.verdict("A", f)) and not cf.verdict("A", f)["copy_failures"])
        assert gates_only == 1264
        pairs = [f for f in fs.by_class["S"] if f.shape == "pair" and f.gate in (6, 10, 12)]
        assert len(pairs) == 296 and fs.skipped["S"] == 8
        assert sum(1 for f in fs.by_class["W"] if f.gate in (6, 10, 12)) == 304
        assert st["msg_c"] == st["msg_borrow"] == 0
    else:
        assert (st["add_blocks"], sum(st["carry"].values()), st["t_sites"]) == (48, 32, 96)
        # the message limbs of the 13-round instance: all 64 through C, each with its 13 a_5 copies,
        # and the a_5 borrow in all 13 x 16 ADD3 blocks
        assert st["msg_c"] == 64 and st["msg_borrow"] == 13 * 16 * 3
        o = int(b.off[1])
        msg = [f for f in fs.by_class["C"] if f.shape == "limb" and 32 <= f.row - o < 96]
        assert sorted(f.row - o for f in msg) == list(range(32, 96))
        for f in msg:
            a5 = [r for c, r, _ in f.writes if c == 5]
            assert len(f.writes) == 16 and len(a5) == 13
            assert sorted((r - o - 164) // 416 for r in a5) == list(range(13))
        touched = {(r - o - 164) // 416 for f in fs.by_class["S"] if f.sub == "a_5" for _, r, _ in f.writes}
        assert touched == set(range(13))


def test_draws_are_indexed_by_the_cell(orc):
    """The drawn bit of a row does not depend on which rows are visited: batch B's window faults
    use the same draw array as a whole-batch walk would, and rows 52 apart draw unrelated bits."""
    fs = cf.faults("A")
    assert fs.bit.shape == (4, cs.batch("A").total) and set(np.unique(fs.bit)) == set(range(16))
    o = int(cs.batch("A").off[3]) + 164
    assert len({int(fs.bit[0, o + 52 * g + 7]) for g in range(8)}) > 2
    for f in fs.by_class["L"][:64]:
        assert f.writes[1][2] == int(cs.batch("A").adv[1, f.row]) ^ (1 << int(fs.bit[0, f.row]))
