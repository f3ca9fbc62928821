"""GPU parity of the permutation-argument prover columns with the CPU restatement
(oracle/permutation.py) at the sizes where the grand product's passes (b2f_gprod.h) and the
factor kernels (b2f_perm.hip) change shape; tests/test_gpu_perm.py compares one 4,096-row block.

Every case compares every written z row 0..usable of every column set (and sigma where asked
for) bit for bit, names the first differing row, and first asserts on the CPU that its shape has
the structure it is named for (chunk / block / scan-run counts from the mirrored constants below,
instance starts inside a chunk, a wave's rows, across a block):

  a  k = 10: a last chunk of one row, one 256-row tile and one more, used == usable;
  b  k = 16: 15-16 blocks of real data, the fused and the two-launch factor passes, row0 != 0;
  c  k = 19: 64 blocks (the one-wave block scan at its largest) and 65 (the 1,024-thread scan);
  d  k = 23: 1,025 and 2,048 blocks (two blocks per scan thread, gp_total's strided loop);
  e  sigma at k = 19 and k = 24 (pm_table_kernel's grid sized by the high table), sampled rows;
  f  full-range u32 cells (field::from_u32) and edge challenges.

The GPU tests need an MI355X (`-m gpu`); the constants mirror is a CPU test."""
import os
import re

import numpy as np
import pytest

import permutation as pm

from conftest import ROOT, random_inputs

gpu = pytest.mark.gpu

# mirrors of b2f_gprod.h (gp::ZC, gp::BLK, gp::SCAN_THREADS, gp::TOT_T) and b2f_perm.hip (LO);
# test_constants_mirror_the_kernels reads them back out of the sources
ZC = 16              # rows per chunk (one lane)
BLK = 256            # chunks per block (one workgroup of gp_chunk / pm_chunk_kernel)
SCAN_THREADS = 1024  # gp_scan's threads above 64 blocks
TOT_T = 256          # gp_total's threads
LO = 1024            # rows per entry of the high coset table OH
WAVE_ROWS = 64 * ZC  # rows a wave of pm_chunk_kernel walks
BLOCK_ROWS = BLK * ZC
R256 = 1 << 256


def n_chunks(usable):
    return -(-usable // ZC)


def n_blocks(usable):
    return -(-n_chunks(usable) // BLK)


def scan_per(nb):
    """Blocks per thread of the 1,024-thread gp_scan."""
    return -(-nb // SCAN_THREADS)


def test_constants_mirror_the_kernels():
    csrc = os.path.join(ROOT, "zk-odst_amd", "csrc")
    with open(os.path.join(csrc, "b2f_gprod.h")) as fh:
        gprod = fh.read()
    with open(os.path.join(csrc, "b2f_perm.hip")) as fh:
        perm = fh.read()

    def const(src, name):
        m = re.findall(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert len(m) == 1, name
        return int(m[0])

    assert const(gprod, "ZC") == ZC
    assert const(gprod, "BLK") == BLK
    assert const(gprod, "SCAN_THREADS") == SCAN_THREADS
    assert const(gprod, "TOT_T") == TOT_T
    assert const(perm, "LO") == LO
    # the one-wave scan's bound and the launch shapes the structure asserts below rely on
    assert "if (nb <= 64)" in gprod and "gp_scan<F, 64>" in gprod
    assert "return (n_chunks(usable) + BLK - 1) / BLK;" in gprod
    assert "const uint64_t per = (nq + T - 1) / T;" in gprod
    assert WAVE_ROWS == 1024 and BLOCK_ROWS == 4096


# ---------------------------------------------------------------------------------------------
# helpers


def _p(form):
    return pm.P_BN254 if form & 2 else pm.P_PALLAS


def _challenges(form, tag):
    p = _p(form)
    rng = np.random.default_rng(1000 + 16 * tag + form)
    return (int.from_bytes(rng.bytes(32), "little") % p, int.from_bytes(rng.bytes(32), "little") % p)


def _limbs(vals, form):
    p = _p(form)
    if form & 1:  # Montgomery form
        vals = [v * R256 % p for v in vals]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)


def _first_diff(got, want):
    """First row at which two [n, 4] limb arrays differ, or None."""
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    return int(bad[0]) if len(bad) else None


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _compare_z(z, zs, usable, form, label=""):
    assert z.shape[0] == len(zs)
    for c, zc in enumerate(zs):
        assert len(zc) == usable + 1
        i = _first_diff(_host(z[c, :usable + 1]), _limbs(zc, form))
        if i is not None:
            pytest.fail("%sz set %d differs first at row %d" % (label, c, i))


def _compare_sigma(sig, sigma, form, label=""):
    for j in range(8):
        i = _first_diff(_host(sig[j]), _limbs(sigma[j], form))
        if i is not None:
            pytest.fail("%ssigma column %d differs first at row %d" % (label, j, i))


class Circuit:
    """A filled batch on the device with its host trace; circuits are instance ranges of it."""

    def __init__(self, engine, n, rounds_choices, seed):
        import b2f
        import torch

        self.batch = b2f.DeviceBatch(random_inputs(n, rounds_choices, seed))
        self.batch.fill(engine)
        engine.sync(torch.cuda.current_stream().cuda_stream)
        self.adv, _ = self.batch.host_trace()
        self.n = self.batch.n
        self._fac = {}

    def rows(self, instances=None):
        """(advice columns of the circuit's rows, its row map from 0)."""
        i0, i1 = instances or (0, self.n)
        off = self.batch.offsets_host[i0:i1 + 1].astype(np.int64)
        return self.adv[:, int(off[0]):int(off[-1])], off - off[0]

    def fac(self, orc, k, form, chunk, beta, gamma, instances=None):
        """pm.factors of a circuit, made once per (field, chunk_len, challenges, circuit)."""
        key = (k, _p(form), chunk, beta, gamma, instances)
        if key not in self._fac:
            cadv, rel = self.rows(instances)
            self._fac[key] = pm.factors(cadv, rel, k, beta, gamma, chunk, _p(form), orc.copies)
        return self._fac[key]

    def run(self, engine, k, usable, form, chunk, beta, gamma, instances=None, sigma=False):
        import torch

        sig, z = self.batch.permutation_columns(engine, k, usable, beta, gamma, chunk_len=chunk,
                                                form=form, instances=instances, sigma=sigma)
        engine.sync(torch.cuda.current_stream().cuda_stream)  # raises on a sticky error
        return sig, z


def _check_fast(engine, orc, circ, k, usable, form, chunk, tag, instances=None, sigma=False):
    """One call against columns_fast: sigma if asked, every z row 0..usable, z closes to 1."""
    beta, gamma = _challenges(form, tag)
    cadv, rel = circ.rows(instances)
    fac = circ.fac(orc, k, form, chunk, beta, gamma, instances)
    sigma_w, zs = pm.columns_fast(cadv, rel, k, usable, beta, gamma, chunk, _p(form), orc.copies,
                                  sigma=sigma, fac=fac)
    assert zs[-1][usable] == 1  # a valid trace closes
    sig, z = circ.run(engine, k, usable, form, chunk, beta, gamma, instances, sigma)
    if sigma:
        _compare_sigma(sig, sigma_w, form)
    _compare_z(z, zs, usable, form)


def _starts(rel):
    return [int(s) for s in rel[:-1]], [int(e) for e in rel[1:]]


# ---------------------------------------------------------------------------------------------
# a. tiny domain

# usable -> (chunks, rows of the last chunk, 256-row tiles of the factor arrays)
TINY = {228: (15, 4, 1), 229: (15, 5, 1), 239: (15, 15, 1), 240: (15, 16, 1), 241: (16, 1, 1),
        255: (16, 15, 1), 256: (16, 16, 1), 257: (17, 1, 2), 1023: (64, 15, 4)}


@pytest.fixture(scope="module")
def tiny(engine):
    return Circuit(engine, 1, (0,), 301)


@gpu
@pytest.mark.parametrize("form,chunk", [(1, 3), (3, 8), (1, 8), (3, 3)])
def test_tiny_domain(engine, orc, tiny, form, chunk):
    """k = 10, one 0-round instance (228 rows): used == usable, a last chunk of 1 / 15 / 16 rows,
    exactly one 256-row tile and one row more, the domain's largest usable. Against `columns`."""
    k = 10
    cadv, rel = tiny.rows()
    used = int(rel[-1])
    assert used == 228 and max(TINY) == (1 << k) - 1 and min(TINY) == used
    beta, gamma = _challenges(form, 1)
    p = _p(form)
    for usable, (nq, last, tiles) in TINY.items():
        assert n_chunks(usable) == nq and usable - ZC * (nq - 1) == last
        assert -(-usable // (ZC * ZC)) == tiles and n_blocks(usable) == 1
        sigma_w, zs = pm.columns(cadv, rel, k, usable, beta, gamma, chunk, p, orc.copies)
        assert zs[-1][usable] == 1
        sig, z = tiny.run(engine, k, usable, form, chunk, beta, gamma, sigma=True)
        label = "usable %d: " % usable
        _compare_sigma(sig, sigma_w, form, label)
        _compare_z(z, zs, usable, form, label)


# ---------------------------------------------------------------------------------------------
# b. several blocks, real data throughout


@pytest.fixture(scope="module")
def blocks(engine):
    # 13 instances, rounds (0, 12, 12, 12, 5, 5, 12, 0, 12, 12, 1, 12, 12): 47,476 rows
    return Circuit(engine, 13, (0, 1, 5, 12, 12, 12), 122)


def _assert_blocks_circuit(rel, usable):
    """Real data over ten or more blocks; instance starts inside a lane's chunk, on a chunk's
    first row, inside a wave's rows, instances across a block boundary and longer than a block."""
    used = int(rel[-1])
    assert 40000 <= used <= 61440 <= usable
    st, en = _starts(rel)
    assert any(s % ZC for s in st)                      # PM_FETCH's refresh inside a chunk
    assert any(s and s % ZC == 0 for s in st)           # ... and at a lane's first row
    assert any(s % WAVE_ROWS for s in st)               # inside a wave: inst_of_wave steps
    assert any(s // BLOCK_ROWS != (e - 1) // BLOCK_ROWS for s, e in zip(st, en))
    assert any(e - s > BLOCK_ROWS for s, e in zip(st, en))
    assert {(e - s - 228) // 416 for s, e in zip(st, en)} == {0, 1, 5, 12}
    assert used // BLOCK_ROWS >= 9


BLOCKS_SHAPE = {61440: (3840, 15, 16), 61441: (3841, 16, 1), (1 << 16) - 7: (4096, 16, 9)}


# form, chunk_len, usable, instances, sigma
@gpu
@pytest.mark.parametrize("form,chunk,usable,instances,sigma", [
    (1, 3, 61440, None, True),
    (3, 1, 61441, None, False),
    (2, 8, (1 << 16) - 7, None, True),
    (0, 4, 61441, None, False),
    (1, 8, 61440, (2, 13), False),
    (3, 3, (1 << 16) - 7, (2, 13), False),
    (1, 1, (1 << 16) - 7, None, False),
    (3, 4, 61440, None, False),
])
def test_several_blocks(engine, orc, blocks, form, chunk, usable, instances, sigma):
    """k = 16, 15 full blocks / one row more / the domain's usual usable: K' of every middle
    block, the fused pass (chunk_len 1 and 3: 8 and 3 chained sets) and the two-launch pass
    (chunk_len 4 and 8) over more than one block, a circuit that starts at trace row 5,448."""
    k = 16
    _, rel = blocks.rows(instances)
    _assert_blocks_circuit(rel, usable)
    if instances:
        assert int(blocks.batch.offsets_host[instances[0]]) > 0
    nq, nb, last = BLOCKS_SHAPE[usable]
    assert (n_chunks(usable), n_blocks(usable), usable - ZC * (nq - 1)) == (nq, nb, last)
    assert 1 < nb <= 64  # the one-wave scan, several blocks
    assert (chunk <= 3) == (chunk in (1, 3))  # PM_CL = 3: the fused pass
    _check_fast(engine, orc, blocks, k, usable, form, chunk, 2, instances, sigma)


@gpu
@pytest.mark.parametrize("form,chunk", [(3, 3), (1, 4)])
def test_usable_ends_inside_an_instances_wave(engine, orc, blocks, form, chunk):
    """usable = used + 5: the last wave of the factor passes starts inside the last instance
    (not the first) and its lanes past `usable` have no row: they must not form a row of their
    own from another instance's context."""
    k = 16
    _, rel = blocks.rows()
    used = int(rel[-1])
    usable = used + 5
    base = (usable - 1) // WAVE_ROWS * WAVE_ROWS  # the last wave of pm_chunk_kernel
    assert int(rel[-2]) <= base < used            # ... starts inside the last instance
    assert n_chunks(usable) % 64                  # ... and has lanes without a chunk
    assert (usable - 1) // 64 * 64 < used and usable % 64  # pm_factor_kernel's last wave too
    _check_fast(engine, orc, blocks, k, usable, form, chunk, 3)


# ---------------------------------------------------------------------------------------------
# c. the scan switch


@pytest.fixture(scope="module")
def scan_circuit(engine):
    # 54 instances, 48 of them 12 rounds: 259,000 rows
    return Circuit(engine, 54, (12,) * 11 + (5, 1, 0), 203)


SCAN_SHAPE = {262144: (16384, 64, 16), 262145: (16385, 65, 1), 266240: (16640, 65, 16)}


@gpu
@pytest.mark.parametrize("form,chunk,usable", [(3, 3, 262144), (3, 3, 262145), (3, 3, 266240),
                                               (1, 8, 262145)])
def test_scan_switch(engine, orc, scan_circuit, form, chunk, usable):
    """k = 19: nb = 64 is the one-wave gp_scan at its largest, nb = 65 the first size of the
    1,024-thread scan (65 threads with one block each), once with a last block of one chunk of
    one row and once with 65 full blocks. Real data through block 63."""
    k = 19
    _, rel = scan_circuit.rows()
    used = int(rel[-1])
    assert 250000 <= used <= 262144
    st, en = _starts(rel)
    assert sum(e - s == 228 + 416 * 12 for s, e in zip(st, en)) > len(st) * 3 // 4
    assert (used - 1) // BLOCK_ROWS == 63
    nq, nb, last = SCAN_SHAPE[usable]
    assert (n_chunks(usable), n_blocks(usable), usable - ZC * (nq - 1)) == (nq, nb, last)
    assert (nb <= 64) == (usable == 262144) and scan_per(nb) == 1
    if usable == 262145:
        assert nq - BLK * (nb - 1) == 1  # the last block: one chunk (of one row)
    if usable == 266240:
        assert nq == BLK * nb
    _check_fast(engine, orc, scan_circuit, k, usable, form, chunk, 4)


# ---------------------------------------------------------------------------------------------
# d. long scans


@pytest.fixture(scope="module")
def four(engine):
    return Circuit(engine, 4, (12,), 401)


LONG_SHAPE = {1024 * 4096 + 1: (262145, 1025, 2, 513), (1 << 23) - 7: (524288, 2048, 2, 1024)}


@gpu
@pytest.mark.parametrize("form,chunk,usable", [(3, 3, 1024 * 4096 + 1), (1, 8, 1024 * 4096 + 1),
                                               (3, 3, (1 << 23) - 7)])
def test_long_scans(orc, four, form, chunk, usable):
    """k = 23: nb = 1,025 (two blocks per scan thread, 513 threads with work, the last with one)
    and nb = 2,048 (every thread two); gp_total strides (nb > 256). Rows 0..used against
    columns_fast on the host, rows used..usable on the device against z[used], the constant
    columns_fast proves for them (its assert: no factor of those rows is zero). An engine of its
    own, closed afterwards: ~1.6 GB of scratch."""
    import b2f
    import torch

    k = 23
    cadv, rel = four.rows()
    used = int(rel[-1])
    assert used == 4 * 5220
    nq, nb, per, busy = LONG_SHAPE[usable]
    assert (n_chunks(usable), n_blocks(usable), scan_per(nb), -(-nb // per)) == (nq, nb, per, busy)
    assert nb > SCAN_THREADS and nb > TOT_T
    p = _p(form)
    beta, gamma = _challenges(form, 5)
    fac = four.fac(orc, k, form, chunk, beta, gamma)
    head = fac.z_head()
    assert head[-1][used] == 1
    assert not pm._tail_has_zero_factor(p, k, used, usable, beta, gamma)
    # columns_fast's own statement of the tail, at a usable small enough to list
    _, zs = pm.columns_fast(cadv, rel, k, used + 3, beta, gamma, chunk, p, orc.copies, sigma=False,
                            fac=fac)
    assert all(zc[:used + 1] == h and zc[used:] == [h[used]] * 4 for zc, h in zip(zs, head))
    eng = b2f.Engine(0)
    try:
        _, z = four.batch.permutation_columns(eng, k, usable, beta, gamma, chunk_len=chunk, form=form,
                                              sigma=False)
        eng.sync(torch.cuda.current_stream().cuda_stream)
        assert z.shape[0] == len(head)
        for c, h in enumerate(head):
            i = _first_diff(_host(z[c, :used + 1]), _limbs(h, form))
            if i is not None:
                pytest.fail("z set %d differs first at row %d" % (c, i))
            want = torch.from_numpy(_limbs([h[used]], form).view(np.int64).copy()).to(z.device)
            bad = (z[c, used:usable + 1] != want).any(dim=1)
            if bool(bad.any()):
                pytest.fail("z set %d differs first at row %d (expected z[used] from there on)"
                            % (c, used + int(torch.nonzero(bad)[0])))
        del z, bad
    finally:
        eng.close()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------
# e. coset tables at scale


def _sigma_samples(k, used, seed):
    n = 1 << k
    n_hi = n // LO
    rng = np.random.default_rng(seed)
    hs = {1, n_hi - 1} | {int(h) for h in rng.integers(1, n_hi, 300)}
    if n_hi > 8 * LO:  # the entries past pm_table_kernel's 8 x 1,024 threads
        hs |= {8 * LO - 1, 8 * LO, 8 * LO + 1}
    rows = set(range(used)) | {n - 1} | {int(r) for r in rng.integers(0, n, 4096)}
    for h in hs:
        rows |= {LO * h - 1, LO * h, LO * h + 1}
    return sorted(rows), hs


@gpu
@pytest.mark.parametrize("k,form", [(19, 1), (19, 2), (24, 3)])
def test_sigma_tables_at_scale(orc, k, form):
    """permutation_sigma on a 2^19 and a 2^24-row domain (OH: 512 and 16,384 entries; above 8,192
    pm_table_kernel's grid is sized by OH): every row of the instances, the rows around a few
    hundred multiples of 1,024 (first and last included), the last row and 4,096 random rows,
    gathered on the device, against delta^c' w^r' by pow."""
    import b2f
    import torch

    p = _p(form)
    n = 1 << k
    n_hi = n // LO
    assert (n_hi > 8 * LO) == (k == 24)
    batch = b2f.DeviceBatch(random_inputs(3, (0, 1, 12), 501 + k))  # offsets only: no witness
    off = batch.offsets_host.astype(np.int64)
    used = int(off[-1])
    rows, hs = _sigma_samples(k, used, 502 + k)
    assert {1, n_hi - 1} <= hs and rows[0] == 0 and rows[-1] == n - 1 and len(hs) > 200
    w, d = pm.domain(p, k)
    maps = [pm.instance_mapping(int(r), orc.copies(int(r))) for r in (off[1:] - off[:-1] - 228) // 416]
    eng = b2f.Engine(0)
    try:
        sig = batch.permutation_sigma(eng, k, form=form)
        eng.sync(torch.cuda.current_stream().cuda_stream)
        idx = torch.tensor(rows, dtype=torch.int64, device=sig.device)
        got = sig.index_select(1, idx).cpu().numpy().view(np.uint64)
        del sig
    finally:
        eng.close()
        torch.cuda.empty_cache()
    inst = np.searchsorted(off, np.asarray(rows), side="right") - 1
    for j in range(8):
        want = []
        for r, t in zip(rows, inst):
            c2, r2 = j, r
            if r < used:
                m = maps[t][j][r - int(off[t])]
                c2, r2 = m >> 29, int(off[t]) + (m & 0x1FFFFFFF)
            want.append(pow(d, c2, p) * pow(w, r2, p) % p)
        i = _first_diff(got[j], _limbs(want, form))
        if i is not None:
            pytest.fail("sigma column %d differs first at row %d" % (j, rows[i]))


# ---------------------------------------------------------------------------------------------
# f. cell and challenge edges

CELL_EDGES = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def small(engine):
    return Circuit(engine, 4, (0, 1, 2), 601)


@pytest.fixture(scope="module")
def wild():
    """A small batch's layout whose advice columns 1..8 hold full-range u32 cells."""
    import b2f
    import torch

    b = b2f.DeviceBatch(random_inputs(4, (0, 1, 2), 601))
    used = b.used_rows
    rng = np.random.default_rng(602)
    cells = rng.integers(0, 1 << 32, (8, used), dtype=np.uint64).astype(np.uint32)
    for j in range(8):
        at = rng.choice(used, 3 * len(CELL_EDGES), replace=False)
        cells[j, at] = np.tile(np.asarray(CELL_EDGES, dtype=np.uint32), 3)
    b.advice.zero_()
    b.advice[1:9, :used] = torch.from_numpy(cells.view(np.int32).copy()).to(b.advice.device)
    torch.cuda.synchronize()
    adv = np.zeros((10, used), dtype=np.uint32)
    adv[1:9] = cells
    return b, adv


@gpu
@pytest.mark.parametrize("form,chunk", [(1, 3), (3, 8), (1, 8), (3, 3)])
def test_full_range_cells(engine, orc, wild, form, chunk):
    """Cells over all of u32 (real a_1..a_8 cells are small) with 0, 1, 2^31 - 1, 2^31 and
    2^32 - 1 in every column: field::from_u32's quotient estimate in both factor kernels.
    Against `columns`, which takes any integer cell; the copies do not hold, so z does not close."""
    import torch

    b, adv = wild
    k, usable = 12, (1 << 12) - 7
    for j in range(1, 9):
        assert set(CELL_EDGES) <= set(int(v) for v in adv[j])
        assert int(adv[j].max()) > 0xF0000000
    assert b.used_rows < usable
    p = _p(form)
    beta, gamma = _challenges(form, 6)
    rel = b.offsets_host.astype(np.int64)
    _, zs = pm.columns(adv, rel, k, usable, beta, gamma, chunk, p, orc.copies)
    _, z = b.permutation_columns(engine, k, usable, beta, gamma, chunk_len=chunk, form=form, sigma=False)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    _compare_z(z, zs, usable, form)


def _edge_challenges(p):
    r = R256 % p
    return {"one_zero": (1, 0), "minus_minus": (p - 1, p - 1), "minus_one": (p - 1, 1),
            "r_rinv": (r, pow(r, p - 2, p))}


@gpu
@pytest.mark.parametrize("which", ["one_zero", "minus_minus", "minus_one", "r_rinv"])
@pytest.mark.parametrize("form", [1, 3])
def test_edge_challenges(engine, orc, small, form, which):
    """(beta, gamma) = (1, 0), (-1, -1), (-1, 1) and (R, 1 / R) on a valid trace, both fields."""
    k = 12
    p = _p(form)
    beta, gamma = _edge_challenges(p)[which]
    cadv, rel = small.rows()
    used = int(rel[-1])
    usable = (1 << k) - 7
    # -1 = w^(n / 2): row 2,048 is the one where (-1, -1) leaves the bare cell as a factor; it
    # lies inside the instances, where the cell is not zero
    assert (1 << (k - 1)) < used <= usable
    # columns_fast first: its asserts show a challenge that makes a factor zero
    _, fz = pm.columns_fast(cadv, rel, k, usable, beta, gamma, 3, p, orc.copies, sigma=False)
    _, zs = pm.columns(cadv, rel, k, usable, beta, gamma, 3, p, orc.copies)
    assert fz == zs and zs[-1][usable] == 1
    _, z = small.run(engine, k, usable, form, 3, beta, gamma)
    _compare_z(z, zs, usable, form)
