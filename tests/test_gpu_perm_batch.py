"""The permutation z columns of many circuits in one call (b2f_permutation_columns_batch_dev):
every circuit's columns are bit for bit what the single call writes for that circuit alone.

Small domains are compared row by row with the CPU restatement (oracle/permutation.py
columns_fast on the circuit's slice of the host trace), large ones with
b2f_permutation_columns_dev (which tests/test_gpu_perm_shapes.py pins to the restatement at
those sizes):

  1  k = 10: four circuits of unequal length inside a batch (instances before the first and
     after the last are skipped), all four forms x chunk_len 3, 1, 8, 5; last chunks of 1..16 rows;
  2  40 circuits x 8 sets = 320 products: more than one block of gp_close, 40 chains;
  3  k = 14: four blocks per product, usable inside a wave, a much shorter last circuit;
  4  k = 17: 8 circuits of 12-round instances against the single call; one timed region;
  5  k = 23: 3 circuits in groups of 2 and 1 (the 2^24-row rule), scratch of one group;
     and 8,200 circuits x 8 sets at k = 10: a pass capped at 65,535 products (8,191 + 9);
  6  k = 19: 65 blocks, the 1,024-thread gp_scan;
  7  a broken copy in one circuit leaves the others' columns alone;
  8  a zero denominator in one circuit: B2F_ERR_FIELD at sync, the others still written;
  9  every argument error of the header's table, then a good call.

Needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

import permutation as pm

from conftest import random_inputs

pytestmark = pytest.mark.gpu

R256 = 1 << 256
R0, R1, R4, R12 = 228, 644, 1892, 5220  # rows of an instance of 0, 1, 4, 12 rounds


def _p(form):
    return pm.P_BN254 if form & 2 else pm.P_PALLAS


def _challenges(form, tag):
    p = _p(form)
    rng = np.random.default_rng(7000 + 16 * tag + form)
    return (int.from_bytes(rng.bytes(32), "little") % p, int.from_bytes(rng.bytes(32), "little") % p)


def _limbs(vals, form):
    p = _p(form)
    if form & 1:  # Montgomery form
        vals = [v * R256 % p for v in vals]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _sets(chunk):
    return (8 + chunk - 1) // chunk


class Trace:
    """A filled batch whose instances have the given rounds, with its host trace."""

    def __init__(self, engine, rounds, seed, host=True):
        import b2f

        x = random_inputs(len(rounds), (0,), seed)
        x["rounds"] = np.asarray(rounds, dtype=np.uint32)
        self.batch = b2f.DeviceBatch(x)
        self.batch.fill(engine)
        engine.sync(_stream())
        self.off = self.batch.offsets_host.astype(np.int64)
        self.adv = self.batch.host_trace()[0] if host else None

    def rows(self, i0, i1):
        off = self.off[i0:i1 + 1]
        return self.adv[:, int(off[0]):int(off[-1])], off - off[0]

    def used(self, first):
        return [int(self.off[b] - self.off[a]) for a, b in zip(first[:-1], first[1:])]


def _check_oracle(engine, orc, tr, first, k, usable, form, chunk, tag):
    """One batch call; every circuit row by row against columns_fast on its slice of the trace;
    every circuit starts at 1 and closes to 1."""
    beta, gamma = _challenges(form, tag)
    z = tr.batch.permutation_columns_batch(engine, k, usable, beta, gamma, first, chunk_len=chunk,
                                           form=form)
    engine.sync(_stream())
    assert tuple(z.shape) == (len(first) - 1, _sets(chunk), 1 << k, 4)
    one = _limbs([1], form)[0]
    got = _host(z[:, :, :usable + 1])
    for c, (a, b) in enumerate(zip(first[:-1], first[1:])):
        cadv, rel = tr.rows(a, b)
        _, zs = pm.columns_fast(cadv, rel, k, usable, beta, gamma, chunk, _p(form), orc.copies,
                                sigma=False)
        assert len(zs) == _sets(chunk) and zs[-1][usable] == 1
        for s, zc in enumerate(zs):
            bad = np.flatnonzero((got[c, s] != _limbs(zc, form)).any(axis=1))
            if len(bad):
                pytest.fail("circuit %d set %d differs first at row %d" % (c, s, int(bad[0])))
        assert (got[c, 0, 0] == one).all() and (got[c, -1, usable] == one).all(), c


# ---------------------------------------------------------------------------------------------
# 1. oracle parity, one block

# a skipped instance, 4 x 0 rounds, 1 + 0 rounds, one of 1 round, one of 0 rounds, a skipped one
TINY_ROUNDS = (1, 0, 0, 0, 0, 1, 0, 1, 0, 0)
TINY_FIRST = (1, 5, 7, 8, 9)


@pytest.fixture(scope="module")
def tiny(engine):
    return Trace(engine, TINY_ROUNDS, 811)


@pytest.mark.parametrize("chunk", [3, 1, 8, 5])
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_batch_equals_oracle_one_block(engine, orc, tiny, form, chunk):
    k, usable = 10, (1 << 10) - 7
    first = list(TINY_FIRST)
    assert first[0] > 0 and first[-1] < len(TINY_ROUNDS)
    assert tiny.used(first) == [4 * R0, R1 + R0, R1, R0] and max(tiny.used(first)) <= usable == 1017
    _check_oracle(engine, orc, tiny, first, k, usable, form, chunk, 1)


@pytest.mark.parametrize("usable,last", [(912, 16), (913, 1), (1008, 16), (1009, 1), (1023, 15)])
def test_batch_last_chunk_rows(engine, orc, tiny, usable, last):
    """usable at the longest circuit's used rows, one row more, and chunks of 16 / 1 / 15 rows at
    the end of the domain."""
    assert usable - 16 * ((usable - 1) // 16) == last and usable <= 16 * 256
    _check_oracle(engine, orc, tiny, list(TINY_FIRST), 10, usable, 3, 3, 2)


# ---------------------------------------------------------------------------------------------
# 2. more than 256 products


@pytest.mark.parametrize("form", [3, 0])
def test_batch_more_than_256_products(engine, orc, form):
    rounds = [int(r) for r in np.random.default_rng(821).integers(0, 2, 40)]
    assert set(rounds) == {0, 1}
    tr = Trace(engine, rounds, 822)
    first = list(range(41))
    assert (len(first) - 1) * _sets(1) == 320 > 256
    _check_oracle(engine, orc, tr, first, 10, (1 << 10) - 7, form, 1, 3)


# ---------------------------------------------------------------------------------------------
# 3. several blocks

BLOCKS_ROUNDS = (4, 4, 4, 1, 4, 4) + (4, 1, 4, 4, 4, 1) + (1,)
BLOCKS_FIRST = (0, 6, 12, 13)


@pytest.fixture(scope="module")
def blocks(engine):
    return Trace(engine, BLOCKS_ROUNDS, 831)


@pytest.mark.parametrize("usable", [(1 << 14) - 7, 12345])
@pytest.mark.parametrize("form", [1, 3])
def test_batch_several_blocks(engine, orc, blocks, form, usable):
    """k = 14: 4 blocks of 4,096 rows per product (3 full and a partial one at 12,345, which ends
    inside a wave's 1,024 rows); circuits of 10,104, 8,856 and 644 rows."""
    first = list(BLOCKS_FIRST)
    assert blocks.used(first) == [5 * R4 + R1, 4 * R4 + 2 * R1, R1]
    assert -(-usable // 4096) == 4 and usable % 1024 and max(blocks.used(first)) <= usable
    _check_oracle(engine, orc, blocks, first, 14, usable, form, 3, 4)


# ---------------------------------------------------------------------------------------------
# 4 - 6. equal to the single call


def _check_single(engine, tr, first, k, usable, form, chunk, tag):
    import torch

    beta, gamma = _challenges(form, tag)
    z = tr.batch.permutation_columns_batch(engine, k, usable, beta, gamma, first, chunk_len=chunk,
                                           form=form)
    engine.sync(_stream())
    for c, (a, b) in enumerate(zip(first[:-1], first[1:])):
        _, z1 = tr.batch.permutation_columns(engine, k, usable, beta, gamma, chunk_len=chunk, form=form,
                                             instances=(a, b), sigma=False)
        engine.sync(_stream())
        assert torch.equal(z[c, :, :usable + 1], z1[:, :usable + 1]), "circuit %d" % c
    return z


K17_COUNTS = (25, 3, 17, 1, 24, 10, 25, 7)


@pytest.fixture(scope="module")
def k17(engine):
    return Trace(engine, (12,) * sum(K17_COUNTS), 841, host=False)


@pytest.mark.parametrize("form,chunk", [(1, 3), (3, 3), (1, 5), (3, 5)])
def test_batch_equals_single_call_k17(engine, k17, form, chunk):
    k, usable = 17, (1 << 17) - 7
    first = [0] + [int(v) for v in np.cumsum(K17_COUNTS)]
    assert len(first) == 9 and max(k17.used(first)) == 25 * R12 <= usable
    _check_single(engine, k17, first, k, usable, form, chunk, 5)
    # one call is one timed region
    beta, gamma = _challenges(form, 5)
    engine.set_timing(True)
    try:
        k17.batch.permutation_columns_batch(engine, k, usable, beta, gamma, first, chunk_len=chunk,
                                            form=form)
        engine.sync(_stream())
        times = engine.kernel_times()
    finally:
        engine.set_timing(False)
    assert times["perm"][1] == 1 and times["perm"][0] > 0, times
    assert all(v[1] == 0 for name, v in times.items() if name != "perm"), times


def test_batch_two_groups_k23(engine):
    """k = 23: 2^24 / usable = 2 circuits per pass, so 3 circuits run as groups of 2 and 1 that
    reuse one scratch; a fresh context takes less than 2.5 x what the single call's takes."""
    import b2f
    import torch

    k, usable, form, chunk = 23, (1 << 23) - 7, 3, 3
    counts = (1600, 1607, 1500)
    tr = Trace(engine, (12,) * sum(counts), 851, host=False)
    first = [0] + [int(v) for v in np.cumsum(counts)]
    assert (1 << 24) // usable == 2 and max(tr.used(first)) <= usable
    assert 24_000_000 < tr.batch.total_rows < 26_000_000
    p = _p(form)
    w, d = pm.domain(p, k)
    beta, gamma = _challenges(form, 6)
    dev = tr.batch.advice.device
    s = _stream()
    n_rows = 1 << k
    z = torch.empty((3, 3, n_rows, 4), dtype=torch.int64, device=dev)
    z1 = torch.empty((3, n_rows, 4), dtype=torch.int64, device=dev)
    taken = {}
    for which in ("batch", "single"):
        eng = b2f.Engine(0)
        try:
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(dev)[0]
            if which == "batch":
                eng.permutation_columns_batch_dev(tr.batch.advice.data_ptr(), tr.batch.total_rows,
                                                  tr.batch.offsets_host, first, k, usable, w, d, beta,
                                                  gamma, chunk, form, z.data_ptr(), n_rows, s)
                eng.sync(s)
                taken[which] = free0 - torch.cuda.mem_get_info(dev)[0]
            else:
                for c in range(3):
                    eng.permutation_columns_dev(tr.batch.advice.data_ptr(), tr.batch.total_rows,
                                                tr.batch.offsets_host[first[c]:first[c + 1] + 1], k,
                                                usable, w, d, beta, gamma, chunk, form, 0,
                                                z1.data_ptr(), n_rows, s)
                    eng.sync(s)
                    if c == 0:
                        taken[which] = free0 - torch.cuda.mem_get_info(dev)[0]
                    assert torch.equal(z[c, :, :usable + 1], z1[:, :usable + 1]), "circuit %d" % c
        finally:
            eng.close()
    del z, z1
    torch.cuda.empty_cache()
    assert 0 < taken["single"] and taken["batch"] < 2.5 * taken["single"], taken


def test_batch_group_capped_by_products(engine):
    """k = 10, chunk_len 1: the 2^24-row rule would put 16,496 circuits in a pass, but a pass
    holds at most 65,535 products (one per blockIdx.y of the grand product's passes), 8,191
    circuits of 8 sets. 8,200 circuits of one 0-round instance run as 8,191 + 9; the circuits on
    both sides of the cut against the single call, every circuit opening and closing at 1."""
    import b2f
    import torch

    k, usable, form, chunk = 10, (1 << 10) - 7, 3, 1
    C = 8200
    assert (1 << 24) // usable > 65535 // _sets(chunk) == 8191 < C
    tr = Trace(engine, (0,) * C, 866, host=False)
    first = list(range(C + 1))
    beta, gamma = _challenges(form, 10)
    eng = b2f.Engine(0)  # 4.5 GB of scratch: a context of its own, closed afterwards
    try:
        z = tr.batch.permutation_columns_batch(eng, k, usable, beta, gamma, first, chunk_len=chunk,
                                               form=form)
        eng.sync(_stream())
        for c in (0, 1, 4095, 8190, 8191, 8192, C - 1):
            _, z1 = tr.batch.permutation_columns(eng, k, usable, beta, gamma, chunk_len=chunk,
                                                 form=form, instances=(c, c + 1), sigma=False)
            eng.sync(_stream())
            assert torch.equal(z[c, :, :usable + 1], z1[:, :usable + 1]), "circuit %d" % c
    finally:
        eng.close()
    one = torch.from_numpy(_limbs([1], form).view(np.int64).copy()).to(z.device)[0]
    assert bool((z[:, 0, 0] == one).all()) and bool((z[:, -1, usable] == one).all())
    del z
    torch.cuda.empty_cache()


def test_batch_second_scan_form_k19(engine):
    """usable = 64 * 4,096 + 1: 65 blocks per product, the 1,024-thread gp_scan."""
    k, usable = 19, 64 * 4096 + 1
    counts = (50, 37)
    tr = Trace(engine, (12,) * sum(counts), 861, host=False)
    first = [0, 50, 87]
    assert -(-(-(-usable // 16)) // 256) == 65 and max(tr.used(first)) <= usable
    _check_single(engine, tr, first, k, usable, 3, 3, 7)
    _check_single(engine, tr, first, k, usable, 1, 5, 7)


# ---------------------------------------------------------------------------------------------
# 7. independence of circuits


def test_batch_broken_copy_stays_in_its_circuit(engine, orc):
    import torch

    rounds = (4, 4) + (4, 1, 1) + (1, 4, 1)
    first = [0, 2, 5, 8]
    tr = Trace(engine, rounds, 871, host=False)
    k, usable, form = 12, (1 << 12) - 7, 1
    assert max(tr.used(first)) <= usable
    one = torch.from_numpy(_limbs([1], form).view(np.int64).copy()).to(tr.batch.advice.device)[0]
    beta, gamma = _challenges(form, 8)
    clean = tr.batch.permutation_columns_batch(engine, k, usable, beta, gamma, first, form=form)
    engine.sync(_stream())
    for c in range(3):
        assert torch.equal(clean[c, 0, 0], one) and torch.equal(clean[c, -1, usable], one), c
    dr, dc, sr, sc = (int(v) for v in orc.copies(4)[100])
    assert 1 <= dc <= 8
    tr.batch.advice[dc, int(tr.off[2]) + dr] ^= 1 << 3  # instance 2: the first of circuit 1
    dirty = tr.batch.permutation_columns_batch(engine, k, usable, beta, gamma, first, form=form)
    engine.sync(_stream())
    for c in (0, 2):
        assert torch.equal(dirty[c, :, :usable + 1], clean[c, :, :usable + 1]), c
        assert torch.equal(dirty[c, -1, usable], one), c
    assert not torch.equal(dirty[1, -1, usable], one)
    assert torch.equal(dirty[1, 0, 0], one)


# ---------------------------------------------------------------------------------------------
# 8. a zero denominator in one circuit


@pytest.mark.parametrize("form", [1, 3])
def test_batch_zero_denominator_in_one_circuit(engine, form):
    import b2f
    import torch

    rounds = (1, 0, 1) + (0, 1, 1) + (1,)
    first = [0, 3, 6, 7]
    tr = Trace(engine, rounds, 881)
    k, usable = 12, (1 << 12) - 7
    p = _p(form)
    w, d = pm.domain(p, k)
    beta = _challenges(form, 9)[0]
    # a cell of circuit 1 on no copy cycle (sigma maps it to itself): column j, circuit row r.
    # The coset term beta delta^j w^r is the same at (j, r) of every circuit, so the cell's value
    # must differ from the other circuits' cell there (zero past their instances), or their
    # factor at (j, r) would be zero too.
    inst = 4
    mp = b2f.permutation_mapping(rounds[inst])
    base = int(tr.off[inst] - tr.off[first[1]])

    def cell(c, j, r):
        row0, used = int(tr.off[first[c]]), int(tr.off[first[c + 1]] - tr.off[first[c]])
        return int(tr.adv[j + 1, row0 + r]) if r < used else 0

    j, ir = next((j, i) for i in range(100, mp.shape[1]) for j in range(8)
                 if int(mp[j, i]) == (j << 29) | i
                 and cell(1, j, base + i) not in (cell(0, j, base + i), cell(2, j, base + i)))
    r = base + ir
    v = cell(1, j, r)
    assert v == int(tr.adv[j + 1, int(tr.off[inst]) + ir])
    gamma = (-(v + beta * pow(d, j, p) * pow(w, r, p))) % p
    s = _stream()

    def single(c, g):
        _, z1 = tr.batch.permutation_columns(engine, k, usable, beta, g, form=form,
                                             instances=(first[c], first[c + 1]), sigma=False)
        return z1

    z0 = single(0, gamma)
    engine.sync(s)  # circuit 0 alone: clean
    single(1, gamma)
    with pytest.raises(b2f.B2FError) as e:
        engine.sync(s)
    assert e.value.code == b2f._lib.ERR_FIELD
    z = tr.batch.permutation_columns_batch(engine, k, usable, beta, gamma, first, form=form)
    with pytest.raises(b2f.B2FError) as e:
        engine.sync(s)
    assert e.value.code == b2f._lib.ERR_FIELD
    engine.sync(s)  # the sticky word is clear
    assert torch.equal(z[0, :, :usable + 1], z0[:, :usable + 1])
    tr.batch.permutation_columns_batch(engine, k, usable, 3, 5, first, form=form)
    engine.sync(s)


# ---------------------------------------------------------------------------------------------
# 9. argument errors


def test_batch_argument_errors(engine, tiny):
    import b2f
    import torch

    L = b2f._lib
    s = _stream()
    b = tiny.batch
    k = 10
    p = pm.P_PALLAS
    w, d = pm.domain(p, k)
    off = b.offsets_host
    n = len(off) - 1
    z = torch.empty((4 * 8 * (1 << k) * 4 + 1,), dtype=torch.int64, device=b.advice.device)
    good = dict(adv=b.advice.data_ptr(), total=b.total_rows, offs=off, first=list(TINY_FIRST), k=k,
                usable=1017, omega=w, delta=d, beta=3, gamma=5, chunk=3, form=1, z=z.data_ptr(),
                out_rows=1 << k)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        engine.permutation_columns_batch_dev(a["adv"], a["total"], a["offs"], a["first"], a["k"],
                                             a["usable"], a["omega"], a["delta"], a["beta"], a["gamma"],
                                             a["chunk"], a["form"], a["z"], a["out_rows"], s)

    bad_off = off.copy()
    bad_off[3] += 4
    cases = [
        ({"adv": 0}, L.ERR_ARG), ({"z": 0}, L.ERR_ARG),                       # null pointers
        ({"first": [2]}, L.ERR_ARG),                                          # no circuits
        ({"first": [1, 5, 5, 8]}, L.ERR_ARG), ({"first": [5, 1]}, L.ERR_ARG),  # not strictly increasing
        ({"first": [1, 5, n + 1]}, L.ERR_ARG),                                # past n
        ({"chunk": 0}, L.ERR_ARG), ({"chunk": 9}, L.ERR_ARG),
        ({"k": 9}, L.ERR_ARG), ({"k": 31}, L.ERR_ARG),
        ({"z": z.data_ptr() + 8}, L.ERR_ARG),                                 # misaligned
        ({"beta": p}, L.ERR_ARG), ({"gamma": p}, L.ERR_ARG), ({"omega": p}, L.ERR_ARG),
        ({"delta": p}, L.ERR_ARG), ({"form": 4}, L.ERR_ARG),
        ({"first": [1, 5, 9]}, L.ERR_ROWS),                                   # circuit 1: 1,744 rows
        ({"usable": 1 << k}, L.ERR_ROWS),
        ({"out_rows": 1017}, L.ERR_ROWS),
        ({"total": int(off[-1]) - 4}, L.ERR_ROWS),
        ({"offs": bad_off}, L.ERR_LAYOUT),
    ]
    for kw, code in cases:
        with pytest.raises(b2f.B2FError) as e:
            call(**kw)
        assert e.value.code == code, (kw, str(e.value))
    with pytest.raises(b2f.B2FError) as e:
        call(first=[1, 5, 9])
    assert "circuit 1" in str(e.value)
    engine.sync(s)  # nothing was launched, nothing is pending
    call()
    engine.sync(s)
