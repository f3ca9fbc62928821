"""CPU check of the lookup z pass's row-run logic (zk-odst_amd/csrc/b2f_lookup.hip): the
rank-order scan's arrays (lk_scan_write: pos, dcnt, the compacted leftover ranks), the per-block
windows (lk_block_kernel: J(p) = p - dcnt[ra(p)] + [p starts a run], the pos-rank and leftover
windows) and the z pass's scatter of those windows into per-row and per-leftover-index tables,
restated in numpy and compared with the definition of halo2's permute_expression_pair
(oracle/lookup.py's restatement): row p's A' rank is the run holding p, a run start takes its
own rank as S', the j-th repeated row takes leftover item n_left - 1 - j.

The kernel's tables hold x_of_rank[r] where this restatement holds r (a relabelling: the z pass
gathers the table in table order). Host logic only; the GPU tests (tests/test_gpu_lookup.py)
compare the kernels' columns with the oracle end to end, including the distributions below."""
import numpy as np
import pytest

TROWS = 1 << 16
LB = 1024


def _scan(count, usable, mult=None):
    """pos, dcnt, leftover multiplicity per rank, compacted leftover ranks and their starts."""
    if mult is None:
        mult = np.ones(TROWS, dtype=np.int64)
        # table row 0's multiplicity (it fills the rows past the table); the kernel gives it to the
        # rank holding table row 0, here rank 0 -- the window logic does not depend on which rank
        mult[0] = usable - TROWS + 1
    pos = np.concatenate([[0], np.cumsum(count)[:-1]])
    dcnt = np.cumsum(count > 0)
    m = mult - (count > 0)
    lrank = np.nonzero(m)[0]
    lstart = np.concatenate([[0], np.cumsum(m[lrank])[:-1]]) if len(lrank) else np.zeros(0, dtype=np.int64)
    return pos, dcnt, m, lrank, lstart


def _last_le(a, v, lim=None):
    a = a if lim is None else a[:lim]
    return int(np.searchsorted(a, v, side="right")) - 1


def _windows(pos, dcnt, lstart, nr, usable, b):
    """lk_block_kernel for block b: (r0, r1, J0, J1, k0, k1)."""
    n_left = usable - int(dcnt[-1])
    base, end = b * LB, min(b * LB + LB, usable)

    def J(p):
        r = _last_le(pos, p)
        return p - int(dcnt[r]) + (1 if pos[r] == p else 0)

    r0, r1 = _last_le(pos, base), _last_le(pos, end - 1)
    J0 = J(base)
    J1 = n_left if end == usable else J(end)
    k0, k1 = 1, 0
    if J1 > J0:
        k0 = _last_le(lstart, n_left - J1, nr)
        k1 = _last_le(lstart, n_left - 1 - J0, nr)
    return r0, r1, J0, J1, k0, k1


def _scatter(pos, dcnt, lrank, lstart, usable, b, win):
    """The z pass's step 1 for block b: (A' rank, S' rank) of every row of the block."""
    r0, r1, J0, J1, k0, k1 = win
    n_left = usable - int(dcnt[-1])
    nr = len(lrank)
    base, end = b * LB, min(b * LB + LB, usable)
    ent = np.full(end - base, -1, dtype=np.int64)
    start = np.zeros(end - base, dtype=bool)
    jrel = np.zeros(end - base, dtype=np.int64)
    for r in range(r0, r1 + 1):
        s0, s1 = int(pos[r]), int(pos[r + 1]) if r + 1 < TROWS else usable
        for q in range(max(s0, base), min(s1, end)):
            ent[q - base] = r
            start[q - base] = q == s0
            jrel[q - base] = q - int(dcnt[r]) - J0
    ylo, yhi = n_left - J1, n_left - J0
    yl = np.full(max(yhi - ylo, 0), -1, dtype=np.int64)
    for kk in range(k0, k1 + 1):
        y0, y1 = int(lstart[kk]), int(lstart[kk + 1]) if kk + 1 < nr else n_left
        for y in range(max(y0, ylo), min(y1, yhi)):
            yl[y - ylo] = lrank[kk]
    assert (ent >= 0).all(), "a row of the block outside its pos window"
    rs = np.where(start, ent, -1)
    for i in np.nonzero(~start)[0]:
        y = yhi - 1 - jrel[i]
        assert 0 <= jrel[i] < J1 - J0 and yl[y - ylo] >= 0, "a leftover index outside its window"
        rs[i] = yl[y - ylo]
    return ent, rs


def _reference(count, usable, mult=None):
    """A' / S' ranks of every row by the definition (run holding the row; run start; the j-th
    repeated row takes leftover item n_left - 1 - j, leftover items in rank order)."""
    a_rank = np.repeat(np.arange(TROWS), count)
    starts = np.zeros(usable, dtype=bool)
    starts[np.concatenate([[0], np.cumsum(count)[:-1]])[count > 0]] = True
    if mult is None:
        m = np.ones(TROWS, dtype=np.int64)
        m[0] = usable - TROWS + 1
    else:
        m = mult.copy()
    m -= count > 0
    items = np.repeat(np.arange(TROWS), m)  # leftover items, ascending
    s_rank = a_rank.copy()
    rep = np.nonzero(~starts)[0]
    s_rank[rep] = items[len(items) - 1 - np.arange(len(rep))]
    return a_rank, s_rank


def _counts(kind, usable, rng):
    if kind == "uniform":
        x = rng.integers(0, TROWS, usable)
    elif kind == "three_values":
        x = rng.choice(np.array([5, 40000, 65535]), usable, p=[0.8, 0.15, 0.05])
    elif kind == "two_runs":
        x = np.where(np.arange(usable) < 100000, 7, 60000)
    else:  # every value once, then repeats of the last
        x = np.concatenate([np.arange(TROWS), np.full(usable - TROWS, TROWS - 1)])
    # ranks: a random order of the table values (the compressed values' sort order)
    rank_of = rng.permutation(TROWS)
    return np.bincount(rank_of[x], minlength=TROWS)


@pytest.mark.parametrize("kind", ["uniform", "three_values", "two_runs", "every_value_once"])
def test_block_windows_equal_definition(kind):
    rng = np.random.default_rng(53)
    usable = (1 << 17) - 7
    count = _counts(kind, usable, rng)
    assert count.sum() == usable
    pos, dcnt, m, lrank, lstart = _scan(count, usable)
    assert int(m.sum()) == usable - int(dcnt[-1])  # leftover items = repeated rows
    a_ref, s_ref = _reference(count, usable)
    nb = (usable + LB - 1) // LB
    # every block of a sample (first, last and some inside), scattered and compared
    for b in sorted({0, 1, nb // 3, nb // 2, nb - 2, nb - 1}):
        win = _windows(pos, dcnt, lstart, len(lrank), usable, b)
        a, s = _scatter(pos, dcnt, lrank, lstart, usable, b, win)
        lo = b * LB
        assert np.array_equal(a, a_ref[lo:lo + len(a)]), (kind, b)
        assert np.array_equal(s, s_ref[lo:lo + len(s)]), (kind, b)


# ---------------------------------------------------------------------------------------------
# Table rows of equal compressed value (a theta with T[x1] = T[x2]): halo2's map holds one key for
# them, so they are one run with one run start and one pool of leftovers. The kernels keep one
# rank per table row; lk_tie_fix_kernel flags the ranks equal to the rank before (PREV) and after
# (NEXT), and rank_run gives a group's head (NEXT alone) the sum of its members' counts and
# multiplicities and the other members (PREV) count 0 and multiplicity 0 -- a state no rank had
# before (an unused rank kept multiplicity >= 1). Below: rank_run restated loop for loop, fed to
# the same _scan / _windows / _scatter as above, against the definition applied to the values.
PREV, NEXT = 1 << 16, 1 << 17
SC_PER, SC_PART = 16, 4096  # ranks per scan thread, per scan workgroup (SC_THREADS * SC_PER)
SAMP = 32


def _flags(val):
    """lk_tie_fix_kernel's group flags from the values in rank order (nondecreasing)."""
    fl = np.zeros(TROWS, dtype=np.int64)
    same = val[1:] == val[:-1]
    fl[1:][same] |= PREV
    fl[:-1][same] |= NEXT
    return fl


def _rank_run(perm, cnt_of_x, usable):
    """rank_run: per rank the count and multiplicity the scan sees. perm = x_of_rank | flags."""
    mult0 = usable - TROWS + 1
    nv = np.zeros(TROWS, dtype=np.int64)
    mv = np.zeros(TROWS, dtype=np.int64)
    for r in range(TROWS):
        w = int(perm[r])
        x = w & 0xFFFF
        nv[r] = cnt_of_x[x]
        mv[r] = mult0 if x == 0 else 1
        if w & PREV:
            nv[r] = mv[r] = 0
        elif w & NEXT:
            q = r + 1
            while q < TROWS and int(perm[q]) & PREV:
                y = int(perm[q]) & 0xFFFF
                nv[r] += cnt_of_x[y]
                mv[r] += mult0 if y == 0 else 1
                q += 1
    return nv, mv


# (first rank, size): sizes 2, 3 and 17; across a scan thread's 16 ranks; across a 4,096-rank part
# (and so a thread and a sample); across a 32-rank sample boundary; the last ranks of the table
GROUPS = [(5, 2), (100, 3), (200, 17), (14, 4), (SC_PART - 2, 5), (2 * SC_PART - 1, 2), (SAMP * 9 - 1, 2),
          (SAMP * 21 - 3, 6), (TROWS - 3, 3)]
ZGROUP = (1000, 3)  # the group that holds table row 0 (head, middle or last member)


def _grouped_case(present, zpos, usable, seed, all_zero=False):
    """val (value id = head rank, per rank), perm (x_of_rank | flags) and the counts by table row."""
    rng = np.random.default_rng(seed)
    groups = GROUPS + [ZGROUP]
    val = np.arange(TROWS)
    for s, n in groups:
        val[s:s + n] = s
    x_of_rank = rng.permutation(TROWS)
    zr = ZGROUP[0] + zpos  # table row 0's rank
    i = int(np.nonzero(x_of_rank == 0)[0][0])
    x_of_rank[i], x_of_rank[zr] = x_of_rank[zr], 0
    if all_zero:
        cnt_rank = np.zeros(TROWS, dtype=np.int64)
        cnt_rank[zr] = usable
    else:
        r = rng.integers(0, TROWS, usable - 200)  # (the groups' forced members take up to 135 rows)
        cnt_rank = np.bincount(r, minlength=TROWS)
        for s, n in groups:  # which members occur among the inputs
            keep = {"all": range(s, s + n), "first": [s], "last": [s + n - 1], "none": [],
                    "mixed": range(s, s + n, 2)}[present]
            for q in range(s, s + n):
                if q in keep:
                    cnt_rank[q] = max(cnt_rank[q], 1 + (q % 3))
                else:
                    cnt_rank[q] = 0
        # keep the total: the difference goes to an ungrouped rank far from the groups
        cnt_rank[30000] += usable - cnt_rank.sum()
        assert cnt_rank[30000] >= 0
    cnt_of_x = np.zeros(TROWS, dtype=np.int64)
    cnt_of_x[x_of_rank] = cnt_rank
    return val, x_of_rank | _flags(val), cnt_of_x, cnt_rank


def _check_grouped(val, perm, cnt_of_x, cnt_rank, usable, blocks=None):
    nv, mv = _rank_run(perm, cnt_of_x, usable)
    # the definition: one run per value; its count and table multiplicity are its rows' sums
    mult_rank = np.where((perm & 0xFFFF) == 0, usable - TROWS + 1, 1)
    gcount = np.bincount(val, weights=cnt_rank, minlength=TROWS).astype(np.int64)
    gmult = np.bincount(val, weights=mult_rank, minlength=TROWS).astype(np.int64)
    assert gcount.sum() == usable and gmult.sum() == usable
    a_ref, s_ref = _reference(gcount, usable, gmult)
    pos, dcnt, m, lrank, lstart = _scan(nv, usable, mv)
    assert (m >= 0).all() and int(m.sum()) == usable - int(dcnt[-1])
    nb = (usable + LB - 1) // LB
    for b in (range(nb) if blocks is None else blocks):
        win = _windows(pos, dcnt, lstart, len(lrank), usable, b)
        a, s = _scatter(pos, dcnt, lrank, lstart, usable, b, win)
        lo = b * LB
        # the kernel's tables hold ranks; equal-valued ranks are the same column value
        assert np.array_equal(val[a], a_ref[lo:lo + len(a)]), b
        assert np.array_equal(val[s], s_ref[lo:lo + len(s)]), b


@pytest.mark.parametrize("usable", [1 << 16, (1 << 17) - 7])
@pytest.mark.parametrize("present", ["all", "first", "last", "none", "mixed"])
def test_equal_value_groups_are_one_run(present, usable):
    """Groups of 2, 3, 6 and 17 ranks, across a thread's 16 ranks, a 4,096-rank part and a
    32-rank sample, one holding table row 0 (as a later member), with every member, only the
    first, only the last, every other or none among the inputs."""
    val, perm, cnt_of_x, cnt_rank = _grouped_case(present, 1, usable, 71)
    # the groups really cross the boundaries named
    for step in (SC_PER, SC_PART, SAMP):
        assert any(s // step != (s + n - 1) // step for s, n in GROUPS), step
    assert {n for _, n in GROUPS} >= {2, 3, 17}
    _check_grouped(val, perm, cnt_of_x, cnt_rank, usable)


@pytest.mark.parametrize("usable", [1 << 16, (1 << 17) - 7])
@pytest.mark.parametrize("zpos", [0, 1, 2])
def test_group_holding_table_row_zero(zpos, usable):
    """Table row 0 (multiplicity usable - 2^16 + 1) as the head, a middle and the last member of
    a group of three: the pooled multiplicity is usable - 2^16 + 3 wherever it sits."""
    val, perm, cnt_of_x, cnt_rank = _grouped_case("all", zpos, usable, 73)
    nv, mv = _rank_run(perm, cnt_of_x, usable)
    s, n = ZGROUP
    assert mv[s] == usable - TROWS + 3 and (mv[s + 1:s + n] == 0).all()
    assert nv[s] == cnt_rank[s:s + n].sum() and (nv[s + 1:s + n] == 0).all()
    nb = (usable + LB - 1) // LB
    _check_grouped(val, perm, cnt_of_x, cnt_rank, usable, blocks=sorted({0, 1, 2, nb // 2, nb - 2, nb - 1}))


@pytest.mark.parametrize("usable", [1 << 16, (1 << 17) - 7])
@pytest.mark.parametrize("zpos", [0, 2])
def test_all_zero_circuit_with_row_zero_in_a_group(zpos, usable):
    """Every row is dense 0 and row 0's value equals other rows': one run covers the circuit, its
    start takes one of the pooled usable - 2^16 + 3 items, every other item goes to a repeated
    row."""
    val, perm, cnt_of_x, cnt_rank = _grouped_case("all", zpos, usable, 79, all_zero=True)
    nb = (usable + LB - 1) // LB
    _check_grouped(val, perm, cnt_of_x, cnt_rank, usable, blocks=sorted({0, 1, nb // 2, nb - 2, nb - 1}))


@pytest.mark.parametrize("usable", [1 << 16, (1 << 16) + 100])
def test_every_rank_in_a_pair(usable):
    """The shape of theta = -1: 32,768 pairs (here offset by one rank, so every 16th pair crosses
    a thread, some a sample and a part), uniform inputs -- members present in every pattern."""
    rng = np.random.default_rng(83)
    val = np.arange(TROWS)
    val[2:TROWS - 1:2] = val[1:TROWS - 2:2]  # pairs (1, 2), (3, 4), ...; ranks 0 and 65535 single
    x_of_rank = rng.permutation(TROWS)
    cnt_of_x = np.bincount(np.concatenate([rng.integers(0, TROWS, 1 << 16),
                                           np.zeros(usable - (1 << 16), dtype=np.int64)]), minlength=TROWS)
    cnt_rank = cnt_of_x[x_of_rank]
    perm = x_of_rank | _flags(val)
    both = (cnt_rank[1:TROWS - 2:2] > 0) & (cnt_rank[2:TROWS - 1:2] > 0)
    assert both.sum() > 1000 and both[7::8].any()  # pairs (15, 16), (31, 32), ... cross a thread
    _check_grouped(val, perm, cnt_of_x, cnt_rank, usable)
