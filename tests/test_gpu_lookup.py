"""GPU parity of the lookup-argument prover columns (b2f_lookup_columns_dev, SURVEY.md §8(f)
row 4) with the CPU restatement of halo2_proofs 0.3.0's lookup prover (oracle/lookup.py):
A, S, A', S' and z bit-exact, in Montgomery and canonical form, for circuits inside the trace,
straddling its end and almost entirely past it; a corrupted lookup cell is reported at its
row. Needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

from conftest import random_inputs

pytestmark = pytest.mark.gpu

R256 = 1 << 256


def _mod(form):
    import lookup as lk

    return lk.P_BN254 if form & 2 else lk.P


def _chal(seed, form=1):
    r = np.random.default_rng(seed)
    return [int.from_bytes(r.bytes(32), "little") % _mod(form) for _ in range(3)]


def _col_ints(t):
    """int64 [rows, 4] limbs -> list of Python ints."""
    a = t.cpu().numpy().view(np.uint64).astype(object)
    return [int(v) for v in (a[:, 0] | (a[:, 1] << 64) | (a[:, 2] << 128) | (a[:, 3] << 192))]


def _circuit_rows(adv, total, begin, usable):
    a = np.zeros((3, usable), dtype=np.uint32)
    n = max(0, min(usable, total - begin))
    a[:, :n] = adv[:3, begin:begin + n]
    return a


@pytest.fixture(scope="module")
def trace(engine):
    import b2f
    import torch

    x = random_inputs(26, (12,), 61)
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    return batch


@pytest.mark.parametrize("form", [1, 0, 3, 2])
def test_lookup_columns_equal_oracle(engine, trace, form):
    """Forms 0/1 pasta Fp, 2/3 BN254 Fr (the reference circuit's field)."""
    import lookup as lk
    import torch

    usable = (1 << 17) - 7
    total = trace.total_rows
    begins = [0, total - 20000, total - 5]
    p = _mod(form)
    theta, beta, gamma = _chal(7 + form, form)
    out, bad = trace.lookup_columns(engine, begins, usable, theta, beta, gamma, form=form)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    assert (bad.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all()
    adv, _ = trace.host_trace()
    for c, b in enumerate(begins):
        a = _circuit_rows(adv, total, b, usable)
        ref = lk.columns(a[0], a[1], a[2], usable, theta, beta, gamma, p)
        assert ref[4][-1] == 1  # a valid lookup closes
        for j, name in enumerate(["A", "S", "A'", "S'", "z"]):
            n = usable + 1 if j == 4 else usable
            got = _col_ints(out[c, j, :n])
            want = ref[j] if form in (0, 2) else [v * R256 % p for v in ref[j]]
            if got != want:
                i = next(i for i in range(n) if got[i] != want[i])
                pytest.fail("circuit %d column %s differs first at row %d" % (c, name, i))


def _groups_present(T, xs):
    """Table rows grouped by equal compressed value, in rank order (value, then table row -- the
    order of lk_tie_fix_kernel): [(first rank, members, members among the inputs xs)] for every
    group of two or more rows, and the number of such groups."""
    order = sorted(range(1 << 16), key=lambda x: (T[x], x))
    have = set(int(v) for v in np.unique(xs))
    out = []
    r = 0
    while r < len(order):
        e = r + 1
        while e < len(order) and T[order[e]] == T[order[r]]:
            e += 1
        if e - r > 1:
            out.append((r, order[r:e], [x for x in order[r:e] if x in have]))
        r = e
    return out


def _pooled(groups):
    """The groups with two or more members among the inputs: where one run (halo2) and one run per
    table row differ."""
    return [g for g in groups if len(g[2]) >= 2]


def _across_chunk(groups, chunk=16):
    """Of those, the groups whose ranks lie in two of the rank scan's 16-rank thread chunks."""
    return [g for g in _pooled(groups) if g[0] // chunk != (g[0] + len(g[1]) - 1) // chunk]


def _assert_case_is_hit(T, xs, n_groups):
    """The CPU-side conditions of a trace-based colliding-theta case: the table has n_groups
    groups, some group has two or more members among the inputs, and one of those lies across a
    16-rank chunk of the rank order. The rank order depends on theta alone, and at theta = -1,
    -3 and -5 every pair starts at an even rank (measured: no pair of the whole table crosses a
    chunk), so no choice of inputs can meet the last condition there; then that fact is asserted
    in its place, and theta = -24 and -33 (2,048 and 3,072 pairs across a chunk) carry it."""
    groups = _groups_present(T, xs)
    assert len(groups) == n_groups
    assert _pooled(groups)
    crossing = [g for g in groups if g[0] // 16 != (g[0] + len(g[1]) - 1) // 16]
    if crossing:
        assert _across_chunk(groups)
    else:
        assert all(r % 2 == 0 and len(m) == 2 for r, m, _ in groups)
    return groups, bool(crossing)


def _limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)


def _run_and_compare(engine, batch, rows_of, begins, usable, theta, beta, gamma, form, label=""):
    """One call for the circuits at `begins`; every circuit's five columns against lk.columns on
    rows_of(circuit) (the first differing row per column reported), first_bad all ones, a clean
    sync (no B2F_ERR_CHECK: the permuted columns' den product equals the num side's) and
    z[usable] = 1."""
    import lookup as lk
    import torch

    p = _mod(form)
    out, bad = batch.lookup_columns(engine, begins, usable, theta, beta, gamma, form=form)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    assert (bad.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all()
    got = out.cpu().numpy().view(np.uint64)
    one = 1 if form in (0, 2) else R256 % p
    diffs = []
    for c in range(len(begins)):
        a = rows_of(c)
        ref = lk.columns(a[0], a[1], a[2], usable, theta, beta, gamma, p)
        assert ref[4][-1] == 1
        for j, name in enumerate(["A", "S", "A'", "S'", "z"]):
            n = usable + 1 if j == 4 else usable
            want = _limbs(ref[j] if form in (0, 2) else [v * R256 % p for v in ref[j]])
            ne = np.nonzero((got[c, j, :n] != want).any(axis=1))[0]
            if len(ne):
                diffs.append("circuit %d column %s differs first at row %d (%d rows differ)"
                             % (c, name, int(ne[0]), len(ne)))
        assert [int(v) for v in got[c, 4, usable]] == lk.to_limbs(one), (label, c)
    if diffs:
        pytest.fail("%s: %s" % (label, "; ".join(diffs)))


@pytest.mark.parametrize("which", ["small", "minus", "mid", "minus3"])
def test_lookup_structured_theta(engine, trace, which):
    """Challenges whose table values share their top 64-bit limb in long runs (round 6): theta =
    3 puts all 2^16 values below 2^192 (one run, already in order), theta = -2^40 puts 65,281 of
    them below 2^192 in descending order of x (a long run out of order), theta = 2^100 + 1 leaves
    runs by tag. The rank order is the order of the full values in every case
    (lk_tie_fix_kernel), so the columns equal the oracle's. The first three keep the 2^16 table
    values distinct; theta = -3 makes 24,576 pairs of table rows equal (T[1] = T[2], T[0] = T[7]),
    which halo2's map pools into one run each: the case is shown to be hit on the CPU (pairs with
    both rows among the circuit's inputs; see _assert_case_is_hit for the 16-rank chunks) before
    the columns are compared."""
    import lookup as lk

    usable = 1 << 16
    theta = {"small": 3, "minus": lk.P - (1 << 40), "mid": (1 << 100) + 1, "minus3": lk.P - 3}[which]
    _, beta, gamma = _chal(13)
    adv, _ = trace.host_trace()
    a = _circuit_rows(adv, trace.total_rows, 5000, usable)
    if which == "minus3":
        _assert_case_is_hit(lk.table_values(theta), a[1], 24576)
    else:
        assert not _groups_present(lk.table_values(theta), a[1])
    _run_and_compare(engine, trace, lambda c: a, [5000], usable, theta, beta, gamma, 1, "theta " + which)


@pytest.mark.parametrize("form,minus", [(1, 1), (0, 1), (1, 5), (0, 5), (3, 3), (1, 24), (3, 33)])
def test_lookup_dense_collisions_on_trace(engine, trace, form, minus):
    """theta = -1 (every table row in a pair, T[2k] = T[2k + 1]), theta = -5 (16,384 pairs) in
    pasta Fp, Montgomery and canonical, and theta = -3 in BN254 Fr (24,576 pairs), on the real
    trace with usable = 2^16 + 100: row 0's multiplicity is 101, and at theta = -1 and -3 it is
    pooled with row 1's / row 7's. Two circuits, one inside the trace and one across its end.
    Shown on the CPU first: over a thousand pairs with both rows among the inputs. At these three
    thetas every pair starts at an even rank, so none can lie across a 16-rank chunk of the rank
    scan whatever the inputs (_assert_case_is_hit); theta = -24 (24,576 pairs, row 0 in one, 2,048
    across a chunk, 1,024 across a 32-rank sample) and theta = -33 in BN254 Fr (16,384 pairs, 3,072
    across a chunk) are the cases where a pooled pair's two ranks belong to two scan threads."""
    import lookup as lk

    p = _mod(form)
    theta = p - minus
    usable = (1 << 16) + 100
    total = trace.total_rows
    begins = [5000, total - 30000]
    _, beta, gamma = _chal(47 + minus, form)
    adv, _ = trace.host_trace()
    rows = [_circuit_rows(adv, total, b, usable) for b in begins]
    T = lk.table_values(theta, p)
    for a in rows:
        groups, crossing = _assert_case_is_hit(T, a[1], {1: 32768, 5: 16384, 3: 24576, 24: 24576, 33: 16384}[minus])
        assert len(_pooled(groups)) > 1000
        assert crossing == (minus in (24, 33))
        if minus in (1, 3, 24):  # row 0 in a pooled group
            assert any(0 in m for _, m, _ in _pooled(groups))
    _run_and_compare(engine, trace, lambda c: rows[c], begins, usable, theta, beta, gamma, form,
                     "theta -%d form %d" % (minus, form))


def _own_batch(xs, rows):
    """A trace whose lookup cells are the dense values xs (then zero rows up to `rows`)."""
    import b2f
    import torch

    rng = np.random.default_rng(59)
    adv = rng.integers(0, 2**32, (10, rows), dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([xs, np.zeros(rows - len(xs), dtype=np.uint32)]).astype(np.uint32)
    adv[0] = np.where(x < 256, 0, np.where(x < 32768, 1, 2)).astype(np.uint32)
    adv[1] = x
    adv[2] = _spread16(x)
    batch = b2f.DeviceBatch(random_inputs(1, (0,), 1), device="cuda:0", total_rows=rows)
    batch.advice.copy_(torch.from_numpy(adv.view(np.int32)))
    return batch, adv


def test_lookup_constructed_pairs(engine):
    """theta = -3, three circuits of exactly 2^16 rows (no padding row adds x = 0) in one call:
    (a) both rows of every one of the 24,576 equal-valued pairs, a quarter of them several times
    -- one run per pair where one rank per table row made two; (b) only the larger row of each
    pair (of {0, 7} only 7): the run and all the pair's leftovers belong to a rank that is not the
    group's first; (c) only the smaller row. In (b) and (c) one run per table row and one run per
    value coincide (shown: no pair has both rows present), in (a) they do not."""
    import lookup as lk

    usable = 1 << 16
    theta = lk.P - 3
    T = lk.table_values(theta)
    pairs = [m for _, m, _ in _groups_present(T, np.zeros(0, dtype=np.uint32))]
    assert len(pairs) == 24576 and all(len(m) == 2 for m in pairs) and [0, 7] in pairs
    lo = np.array([min(m) for m in pairs], dtype=np.uint32)
    hi = np.array([max(m) for m in pairs], dtype=np.uint32)
    rng = np.random.default_rng(61)
    both = np.concatenate([lo, hi])
    xs = [np.concatenate([both, rng.choice(both, usable - len(both))]),
          np.concatenate([hi, rng.choice(hi, usable - len(hi))]),
          np.concatenate([lo, rng.choice(lo, usable - len(lo))])]
    xs = [rng.permutation(x).astype(np.uint32) for x in xs]
    assert len(_pooled(_groups_present(T, xs[0]))) == 24576
    assert not _pooled(_groups_present(T, xs[1])) and 0 not in xs[1] and 7 in xs[1]
    assert not _pooled(_groups_present(T, xs[2])) and 0 in xs[2] and 7 not in xs[2]
    batch, adv = _own_batch(np.concatenate(xs), 3 * usable)
    _, beta, gamma = _chal(67)
    _run_and_compare(engine, batch, lambda c: adv[:3, c * usable:(c + 1) * usable],
                     [0, usable, 2 * usable], usable, theta, beta, gamma, 1, "pairs a/b/c")


def test_lookup_three_values_two_equal(engine):
    """Exactly three distinct dense values, 1, 2 and 9, at theta = -3: T[1] = T[2] = p - 2 pool
    into one run, T[9] stands alone; a block's rows span thousands of unused ranks, among them
    the equal-valued pairs that no input uses."""
    import lookup as lk

    usable = 1 << 16
    theta = lk.P - 3
    T = lk.table_values(theta)
    assert T[1] == T[2] == lk.P - 2 and T[9] not in (T[1], T[0])
    rng = np.random.default_rng(71)
    xs = rng.choice(np.array([1, 2, 9], dtype=np.uint32), usable, p=[0.5, 0.3, 0.2])
    pooled = _pooled(_groups_present(T, xs))
    assert len(pooled) == 1 and sorted(pooled[0][1]) == [1, 2]
    batch, adv = _own_batch(xs, usable)
    _, beta, gamma = _chal(73)
    _run_and_compare(engine, batch, lambda c: adv[:3, :usable], [0], usable, theta, beta, gamma, 1,
                     "values 1, 2, 9")


def test_lookup_circuit_past_trace_equal_zero_value(engine, trace):
    """Circuits that begin at the trace's end and past it, theta = -3: every row is the zero row
    and T[0] = T[7] = 0, so one pooled run covers all rows: its start takes one of the pooled 102
    items of value 0, the other 101 and every other table row's item go to repeated rows."""
    import lookup as lk

    usable = (1 << 16) + 100
    theta = lk.P - 3
    total = trace.total_rows
    T = lk.table_values(theta)
    assert T[0] == T[7] == 0
    zero = np.zeros((3, usable), dtype=np.uint32)
    _, beta, gamma = _chal(79)
    _run_and_compare(engine, trace, lambda c: zero, [total, total + 12345], usable, theta, beta, gamma, 1,
                     "past the trace")


def _sqrt_mod(a, p):
    """A square root of a modulo the prime p (Tonelli-Shanks), or None."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


def test_lookup_single_collision_random_limbs(engine):
    """BN254 Fr, Montgomery form, theta a root of theta^2 dtag + theta dx + dspread = 0 for table
    rows 255 and 256 (across the tag boundary: dtag = dx = 1, dspread = 43,691): exactly these two
    rows compress to one value and every other value's limbs are as good as random, so the tie
    path sees a run of exactly two fully equal values. Both rows occur among the inputs."""
    import lookup as lk

    p = lk.P_BN254
    ds = lk.spread(256) - lk.spread(255)
    assert lk.tag(256) - lk.tag(255) == 1 and ds == 43691
    root = _sqrt_mod(1 - 4 * ds, p)
    assert root is not None and root * root % p == (1 - 4 * ds) % p
    inv2 = pow(2, p - 2, p)
    thetas = [(-1 + root) * inv2 % p, (-1 - root) * inv2 % p]
    single = [th for th in thetas if len(set(lk.table_values(th, p))) == (1 << 16) - 1]
    assert single
    theta = single[0]
    T = lk.table_values(theta, p)
    assert T[255] == T[256]
    usable = (1 << 16) + 100
    rng = np.random.default_rng(83)
    xs = rng.integers(0, 1 << 16, usable).astype(np.uint32)
    xs[rng.choice(usable, 9, replace=False)] = np.array([255, 256, 256, 255, 255, 256, 255, 255, 256], dtype=np.uint32)
    groups = _groups_present(T, xs)
    assert len(groups) == 1 and sorted(groups[0][1]) == [255, 256] and len(_pooled(groups)) == 1
    rows = (usable + 3) // 4 * 4
    batch, adv = _own_batch(xs, rows)
    _, beta, gamma = _chal(89, 3)
    _run_and_compare(engine, batch, lambda c: adv[:3, :usable], [0], usable, theta, beta, gamma, 3,
                     "rows 255 = 256")


def test_lookup_min_usable_and_bad_row(engine, trace):
    """usable = 2^16 (the table exactly fills the circuit); a flipped spread cell in the trace
    is reported at its circuit row (and only for the circuits holding it)."""
    import lookup as lk
    import torch

    usable = 1 << 16
    theta, beta, gamma = _chal(11)
    out, bad = trace.lookup_columns(engine, [3 * usable], usable, theta, beta, gamma)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    adv, _ = trace.host_trace()
    a = _circuit_rows(adv, trace.total_rows, 3 * usable, usable)
    ref = lk.columns(a[0], a[1], a[2], usable, theta, beta, gamma)
    assert _col_ints(out[0, 3, :usable]) == [v * R256 % lk.P for v in ref[3]]
    assert _col_ints(out[0, 4, :usable + 1]) == [v * R256 % lk.P for v in ref[4]]
    row = 70000
    saved = trace.advice[2, row].item()
    trace.advice[2, row] = saved ^ 0x10
    try:
        out, bad = trace.lookup_columns(engine, [0, 60000, 71000], usable, theta, beta, gamma)
        engine.sync(torch.cuda.current_stream().cuda_stream)
        b = bad.cpu().numpy().view(np.uint64)
        assert int(b[0]) == 2**64 - 1 and int(b[1]) == row - 60000 and int(b[2]) == 2**64 - 1
    finally:
        trace.advice[2, row] = saved


def test_lookup_argument_errors(engine, trace):
    """Argument checks of b2f_lookup_columns_dev (all before any launch)."""
    import lookup as lk
    import torch

    import b2f

    dev = trace.advice.device
    rb = torch.zeros(1, dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int64, device=dev)
    u = 1 << 16
    out = torch.empty((1, 5, u + 1, 4), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(usable=u, theta=3, form=1, out_rows=u + 1):  # noqa: E306
        engine.lookup_columns_dev(trace.advice.data_ptr(), trace.total_rows, rb.data_ptr(), 1,
                                  usable, theta, 5, 7, form, out.data_ptr(), out_rows,
                                  bad.data_ptr(), s)

    for kw, code in [({"usable": u - 1}, b2f._lib.ERR_ROWS), ({"out_rows": u}, b2f._lib.ERR_ROWS),
                     ({"theta": lk.P}, b2f._lib.ERR_ARG), ({"form": 4}, b2f._lib.ERR_ARG),
                     ({"theta": lk.P_BN254, "form": 3}, b2f._lib.ERR_ARG)]:
        with pytest.raises(b2f.B2FError) as e:
            call(**kw)
        assert e.value.code == code, kw
    call()  # valid arguments still run
    engine.sync(s)


@pytest.mark.parametrize("form", [1, 0, 3, 2])
def test_spread_table_columns(engine, form):
    """VERDICT r1 missing 5: the spread table as the prover's three table columns
    (SpreadTableChip::load), rows past 2^16 the row-0 default, in every field form; the
    table side S of the lookup columns is its theta-compression."""
    import lookup as lk
    import torch

    usable = (1 << 16) + 300
    out = engine.spread_table(usable, form)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    p = _mod(form)
    got = out.cpu().numpy().view(np.uint64)
    tag = [lk.tag(x) for x in range(1 << 16)] + [0] * 300
    dense = list(range(1 << 16)) + [0] * 300
    spread = [lk.spread(x) for x in range(1 << 16)] + [0] * 300
    for c, col in enumerate((tag, dense, spread)):
        if form & 1:
            want = np.array([lk.to_limbs(v * R256 % p) for v in col], dtype=np.uint64)
        else:
            want = np.zeros((usable, 4), dtype=np.uint64)
            want[:, 0] = col
        assert np.array_equal(got[c], want), c


@pytest.mark.parametrize("form,which", [(1, "beta"), (3, "beta"), (1, "gamma")])
def test_lookup_zero_factor_reported_then_clean(engine, trace, form, which):
    """beta = -A[row] makes (A + beta) and (A' + beta) zero for that row's value, and
    gamma = -T[x] makes (S + gamma) and (S' + gamma) zero for table row x, so the den total is
    zero: the call reports B2F_ERR_FIELD at b2f_sync (D = the num side's product, lk_nscan_kernel
    on the side stream), and the next call with sound challenges syncs clean -- with no
    B2F_ERR_CHECK, i.e. the permuted columns' den product equals the num side's D -- and its z
    ends at one (N / D by construction; the sync is the check that matters)."""
    import lookup as lk
    import torch

    import b2f

    s = torch.cuda.current_stream().cuda_stream
    usable = (1 << 17) - 7
    p = _mod(form)
    theta, _, gamma = _chal(19, form)
    adv, _ = trace.host_trace()
    row = 1234
    a = lk.compress(theta, int(adv[0, row]), int(adv[1, row]), int(adv[2, row]), p)
    beta = (p - a) % p
    if which == "gamma":  # table row 40,000 (not necessarily among the inputs)
        _, beta, _ = _chal(19, form)
        x = 40000
        gamma = (p - lk.compress(theta, lk.tag(x), x, lk.spread(x), p)) % p
    out, bad = trace.lookup_columns(engine, [0], usable, theta, beta, gamma, form=form)
    with pytest.raises(b2f.B2FError) as e:
        engine.sync(s)
    assert e.value.code == b2f._lib.ERR_FIELD
    if which == "gamma":
        gamma = (gamma + 1) % p
    else:
        beta = (beta + 1) % p
    out, bad = trace.lookup_columns(engine, [0], usable, theta, beta, gamma, form=form)
    engine.sync(s)
    z = _col_ints(out[0, 4, usable:usable + 1])[0]
    one = 1 if form in (0, 2) else R256 % p
    assert z == one  # a valid lookup closes to 1


def test_lookup_group_of_circuits_equal_oracle(engine, trace):
    """Five circuits in one call, one group: each circuit's num block products, their prefix and
    D^-1 come from the trace on the side stream (lk_npart_kernel, lk_nscan_kernel) while the count
    and rank-scan passes run, and one z pass (lk_zpass_kernel, a den-side look-back per circuit)
    covers the group. Every circuit's five columns equal the restatement, BN254 Montgomery form."""
    import lookup as lk
    import torch

    form = 3
    usable = (1 << 16) + 100
    total = trace.total_rows
    begins = [0, 70001, 2 * usable, total - 40000, total - 3]
    p = _mod(form)
    theta, beta, gamma = _chal(23, form)
    out, bad = trace.lookup_columns(engine, begins, usable, theta, beta, gamma, form=form)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    assert (bad.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all()
    adv, _ = trace.host_trace()
    for c, b in enumerate(begins):
        a = _circuit_rows(adv, total, b, usable)
        ref = lk.columns(a[0], a[1], a[2], usable, theta, beta, gamma, p)
        for j in (2, 3, 4):  # A', S' and z (A and S are per-row maps, covered above)
            n = usable + 1 if j == 4 else usable
            got = _col_ints(out[c, j, :n])
            want = [v * R256 % p for v in ref[j]]
            assert got == want, (c, j)


def test_lookup_two_groups_equal_within_call(engine, trace):
    """More circuits than one group holds (at most 2^24 rows per group: 16 circuits of 2^20
    rows), so the call loops over two groups, each forking its own num-side chain (block
    products, prefix, D^-1) to the side stream at its start and reusing the count / NK /
    look-back scratch of the group before (the S part of the block products is computed once, by
    the first group). Circuit 16 (group 2) repeats circuit 5's rows (group 1): all five columns
    bit-identical, the sync clean (no B2F_ERR_CHECK) and every z ends at one (Montgomery form). A
    group that read the previous group's counts, NK or look-back state would differ."""
    import torch

    form = 1
    usable = 1 << 20
    begins = [i * 8000 for i in range(16)] + [5 * 8000]  # inside the 135,720-row trace
    theta, beta, gamma = _chal(31, form)
    out, bad = trace.lookup_columns(engine, begins, usable, theta, beta, gamma, form=form)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    assert (bad.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all()
    one = R256 % _mod(form)
    for c in range(len(begins)):
        assert _col_ints(out[c, 4, usable:usable + 1])[0] == one, c
    # columns A .. S' hold `usable` rows, z usable + 1 (the row after A .. S' is never written)
    assert torch.equal(out[16, :4, :usable], out[5, :4, :usable])
    assert torch.equal(out[16, 4, :usable + 1], out[5, 4, :usable + 1])
    assert not torch.equal(out[16, 2, :usable], out[4, 2, :usable])


def _spread16(x):
    x = x.astype(np.uint32)
    x = (x | (x << 8)) & np.uint32(0x00FF00FF)
    x = (x | (x << 4)) & np.uint32(0x0F0F0F0F)
    x = (x | (x << 2)) & np.uint32(0x33333333)
    x = (x | (x << 1)) & np.uint32(0x55555555)
    return x


def test_lookup_sparse_values_wide_windows(engine):
    """Dense-cell distributions that stretch the z pass's per-block windows (lk_block_kernel):
    three distinct values (a block's rows then span thousands of unused table ranks in rank
    order, the scatter's loops past their first four ranks per thread), two runs of 100,000 and
    31,065 rows (one rank covers every row of many blocks), and every table value once followed
    by 65,529 repeats of 65,535 (leftover items of nearly every rank, the leftover windows at
    their widest). All five columns equal the restatement."""
    import b2f
    import lookup as lk
    import torch

    usable = (1 << 17) - 7
    rng = np.random.default_rng(41)
    xs = [rng.choice(np.array([5, 40000, 65535], dtype=np.uint32), usable, p=[0.8, 0.15, 0.05]),
          np.where(np.arange(usable) < 100000, 7, 60000).astype(np.uint32),
          np.concatenate([rng.permutation(65536).astype(np.uint32),
                          np.full(usable - 65536, 65535, dtype=np.uint32)])]
    rows = (3 * usable + 3) // 4 * 4  # a trace holds a multiple of 4 rows
    adv = rng.integers(0, 2**32, (10, rows), dtype=np.uint64).astype(np.uint32)
    x = np.concatenate(xs + [np.zeros(rows - 3 * usable, dtype=np.uint32)])
    adv[0] = np.where(x < 256, 0, np.where(x < 32768, 1, 2)).astype(np.uint32)
    adv[1] = x
    adv[2] = _spread16(x)
    batch = b2f.DeviceBatch(random_inputs(1, (0,), 1), device="cuda:0", total_rows=rows)
    batch.advice.copy_(torch.from_numpy(adv.view(np.int32)))
    theta, beta, gamma = _chal(43)
    out, bad = batch.lookup_columns(engine, [0, usable, 2 * usable], usable, theta, beta, gamma)
    engine.sync(torch.cuda.current_stream().cuda_stream)
    assert (bad.cpu().numpy().view(np.uint64) == np.uint64(2**64 - 1)).all()
    for c in range(3):
        a = adv[:3, c * usable:(c + 1) * usable]
        ref = lk.columns(a[0], a[1], a[2], usable, theta, beta, gamma)
        for j in range(5):
            n = usable + 1 if j == 4 else usable
            got = _col_ints(out[c, j, :n])
            want = [v * R256 % lk.P for v in ref[j]]
            if got != want:
                i = next(i for i in range(n) if got[i] != want[i])
                pytest.fail("circuit %d column %d differs first at row %d" % (c, j, i))
