"""tests/structured_inputs.py pinned on the CPU: f_ref against references outside this repository
(the EIP-152 vector, the rounds-0 cases, hashlib.blake2b), the oracle against f_ref on every
instance of the structured batch, the oracle's own verdict on its trace, the census (every class
reached on the oracle's trace, counted a second way from g_trace; none of the word-wide classes
reached by uniform inputs on the same row map) and the gate polynomials of
tests/quotient_gates_ref.py over Fp on the blocks the census returns.

CPU only."""
import hashlib

import numpy as np
import pytest

import quotient_gates_ref as gr
import structured_inputs as si

from conftest import random_inputs, words


@pytest.fixture(scope="module")
def ref(orc):
    return si.reference()


def _hex(hw):
    return b"".join(int(w).to_bytes(8, "little") for w in hw).hex()


def test_f_ref_golden_vectors(golden):
    k = golden["kat"]
    assert _hex(si.f_ref(k["rounds"], words(k["h"]), words(k["m"]), words(k["t"]), k["f"])) == k["expected"]
    assert len(golden["rounds0"]) == 6
    for c in golden["rounds0"]:
        assert _hex(si.f_ref(0, words(c["h"]), words(c["m"]), words(c["t"]), c["f"])) == c["expected"], c["name"]


def _blake2b_by_f_ref(data):
    """Unkeyed 64-byte BLAKE2b of `data`, chained by f_ref alone (RFC 7693 section 3.3)."""
    h = list(si.IV)
    h[0] ^= 0x01010040
    nb = max(1, -(-len(data) // 128))
    padded = data.ljust(nb * 128, b"\0")
    for i in range(nb):
        m = [int.from_bytes(padded[128 * i + 8 * j:128 * i + 8 * j + 8], "little") for j in range(16)]
        last = i == nb - 1
        h = si.f_ref(12, h, m, [len(data) if last else 128 * (i + 1), 0], int(last))
    return bytes.fromhex(_hex(h))


@pytest.mark.parametrize("byte", [0x00, 0xff])
def test_f_ref_chains_equal_hashlib(byte):
    for n in (0, 1, 127, 128, 129, 256):
        data = bytes([byte]) * n
        assert _blake2b_by_f_ref(data) == hashlib.blake2b(data).digest(), (byte, n)


def test_g_trace_equals_f_ref_and_solved_targets():
    x = si.batch()
    for i in (0, 1, 7, 191, 500, 1520, len(x) - 1):
        r = x[i]
        _, halves, out = si.g_trace(int(r["rounds"]), r["h"], r["m"], r["t"], int(r["f"]))
        assert len(halves) == 16 * int(r["rounds"])
        assert out == si.f_ref(int(r["rounds"]), r["h"], r["m"], r["t"], int(r["f"]))
    for name in si.SPECIALS:
        assert si.solved_ok(name), "the solved instance %s misses its target" % name


def test_batch_layout():
    x = si.batch()
    assert len(x) == si.N_BATCH == 2002 and x.dtype.itemsize == 216
    assert np.array_equal(x, si.batch()), "batch() is not deterministic"
    at = si.special_positions()
    assert min(at) == 0 and max(at) == len(x) - 1
    assert sum(100 <= i < 1000 for i in at) >= 8 and sum(i > 1500 for i in at) >= 8
    assert set(at.values()) == set(si.SPECIALS)
    assert set(int(r) for r in x["rounds"]) == set(si.ROUNDS)
    assert set(int(f) for f in x["f"]) == {0, 1}
    pat = [i for i in range(len(x)) if i not in at]
    for p in si.PATTERNS:
        assert any(int(x["h"][i][0]) == p for i in pat) and any(int(x["m"][i][0]) == p for i in pat)
    # every (h, m) pattern pair with every kind of t
    seen = set()
    for i in pat:
        h, m, t = int(x["h"][i][3]), int(x["m"][i][9]), (int(x["t"][i][0]), int(x["t"][i][1]))
        kinds = [k for k in si.T_KINDS if si._t_words(k, h, m) == t]
        assert kinds, i
        seen.update((h, m, k) for k in kinds)
    assert len(seen) >= len(si.PATTERNS) ** 2 * len(si.T_KINDS)
    # a special is not at an instance boundary of its own kind: its neighbours are pattern instances
    for i in at:
        assert all(j not in at for j in (i - 1, i + 1))


def test_oracle_equals_f_ref_on_every_instance(orc, ref):
    x = ref.inputs
    bad = []
    for i, r in enumerate(x):
        want = [int(w) for w in ref.h_ref[i]]
        got_c = [int(w) for w in orc.compress(int(r["rounds"]), r["h"], r["m"], r["t"], int(r["f"]))]
        got_f = [int(w) for w in ref.h_out[i]]
        if got_c != want or got_f != want:
            bad.append(i)
    assert not bad, "the oracle's h' differs from f_ref at instances %s" % bad[:10]


def test_oracle_reports_its_trace_clean(ref):
    assert ref.clean["first_failure"] == si.M64
    used = int(sum(228 + 416 * int(r) for r in ref.inputs["rounds"]))
    assert ref.clean["rows_checked"] == ref.total == used + si.PAD_ROWS
    assert not ref.adv[:, used:].any() and not ref.fixed[used:].any()
    assert ref.clean["lookup_failures"] == ref.clean["copy_failures"] == ref.clean["fixed_failures"] == 0
    assert not any(ref.clean["gate_failures"])


def test_census_reaches_every_class(ref):
    """The condition that keeps the GPU comparison from passing vacuously: on the oracle's trace
    of batch(), every class holds at least one block; and the counts are the ones g_trace gives
    from the inputs alone."""
    counts = {c: len(ref.census[c]) for c in si.CLASSES}
    print("census of the structured batch:", counts)
    empty = [c for c in si.CLASSES if counts[c] == 0]
    assert not empty, "batch() no longer reaches %s" % empty
    assert counts == si.expected_census(ref.inputs)


def test_uniform_inputs_reach_no_word_class(orc, ref):
    x = random_inputs(ref.n, (12,), 5)
    x["rounds"] = ref.inputs["rounds"]
    ox = np.frombuffer(x.tobytes(), dtype=orc.INPUT_DTYPE).copy()
    adv, fixed, _, off = orc.fill(ox, total_rows=ref.total)
    assert np.array_equal(off, ref.off) and np.array_equal(fixed, ref.fixed)
    got = si.census(adv, fixed)
    counts = {c: len(got[c]) for c in si.CLASSES}
    print("census of uniform inputs on the same row map:", counts)
    assert all(counts[c] == 0 for c in si.WORD_CLASSES), (
        "uniform inputs reached a whole-word extreme (%r): each has probability 2^-64 per block, "
        "which is why the structured batch exists -- uniform draws never compare the kernels with "
        "the oracle at these values" % counts)


def test_oracle_rejects_every_aimed_fault(ref):
    """The faults the GPU file aims at the extreme blocks: every class has some, a carry of 2 is
    among them, the oracle rejects each one, and the trace is left as it was."""
    before = (ref.adv.copy(), ref.fixed.copy())
    cases = si.faults(ref.census, ref.adv)
    print("%d faults" % len(cases))
    assert 100 <= len(cases) <= 200
    assert {c[0] for c in cases} == set(si.CLASSES)
    assert any(col == 9 and mask == 2 for _, col, _, mask in cases)
    for cls, col, row, mask in cases:
        rep = ref.verdict(col, row, mask)
        assert rep["first_failure"] != si.M64 and rep["first_failure"] >> 8 <= row, (cls, col, row, mask)
        assert rep["rows_checked"] == ref.total
    assert np.array_equal(before[0], ref.adv) and np.array_equal(before[1], ref.fixed)
    # the windowed verdict is the whole trace's: shown on the first and the last fault
    for cls, col, row, mask in (cases[0], cases[-1]):
        ref.adv[col, row] ^= np.uint32(mask)
        try:
            whole = ref.orc.evaluate(ref.adv, ref.fixed, ref.off)
        finally:
            ref.adv[col, row] ^= np.uint32(mask)
        assert whole == ref.verdict(col, row, mask)


def test_gates_vanish_over_fp_on_the_extreme_blocks(orc, ref):
    """A second statement of the gates, apart from orc_eval: on up to 24 blocks of each class
    (first and last ones), every polynomial of every selector that is on at the block's first row
    is 0 modulo the pallas prime; with the carry or a result limb altered it is not."""
    p = orc.MODULI[orc.PALLAS]
    adv, fixed = ref.adv, ref.fixed

    def residues(row, cells, base=0):
        def a(c, j):
            return int(cells[c, row - base + j])

        out = []
        for g in range(16):
            if (int(fixed[row]) >> g) & 1:
                polys = [a(1, 0) - (int(fixed[row]) >> 16)] if g == 14 else gr.GATES[g](a)
                out += [v % p for v in polys]
        return out

    checked = 0
    for cls in si.CLASSES:
        rows = ref.census[cls]
        for r in sorted(set(int(v) for v in np.concatenate([rows[:12], rows[-12:]]))):
            res = residues(r, adv)
            assert res and not any(res), (cls, r)
            checked += 1
    assert 100 <= checked <= 13 * 24
    altered = 0
    for cls, col, row, mask in si.faults(ref.census, adv):
        if not cls.startswith("add"):
            continue  # the XOR gates read the spread cells; a_1 there is the lookup's to pin
        start = max(int(v) for v in ref.census[cls] if v <= row)
        bad = adv[:, start:start + 4].copy()
        bad[col, row - start] ^= np.uint32(mask)
        assert any(residues(start, bad, start)), (cls, col, row, mask)
        altered += 1
    assert altered >= 30
