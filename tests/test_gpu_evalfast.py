"""The eval's fast clean-check pass (eval_hr_kernel / eval_edge_kernel, csrc/b2f_fused.hip) in
front of the exact eval kernel: a clean trace must cost the fast pass only (the exact kernel is
skipped by its device-side gate), and any corruption the pass sees must hand the trace to the exact
kernel, whose report then equals the oracle's. The fast pass checks a wave's band of consecutive
half-round tiles with the limb table (the state words' canonical cells as the half-round starts)
carried from the previous tile's staging; the cases below put faults in those carried cells, at band
and instance boundaries, on mixed rounds (bands that cross instances). Needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

from conftest import random_inputs
from verdict_util import FIXED_COL, INIT_ROWS, NONE, ROUND_ROWS, dev_flip, oracle_window, rounds_of

pytestmark = pytest.mark.gpu

G_ROWS = 52


def _dev_eval(engine, batch, adv, fixed):
    import torch

    batch.advice.copy_(torch.from_numpy(adv.view(np.int32)).to(batch.advice.device))
    batch.fixed.copy_(torch.from_numpy(fixed.view(np.int32)).to(batch.fixed.device))
    batch.evaluate(engine)
    path = engine.debug_eval_path()
    return path, batch.report_dict()


def _canon_rows(off, rounds, hr):
    """Instance-local rows of the canonical state cells as half-round hr (>= 1) starts (a2 / b2 /
    c2 / d2 blocks of the G's of half-round hr - 1; LAYOUT.md, b2f_layout.h canon_state)."""
    hp = hr - 1
    rp = hp >> 1
    rows = []
    for g4 in range(4):
        g = g4 + 4 * (hp & 1)
        gb = INIT_ROWS + ROUND_ROWS * rp + G_ROWS * g
        rows += [(1, gb + 28), (2, gb + 28 + 3), (7, gb + 44), (8, gb + 46), (1, gb + 40 + 1),
                 (2, gb + 32 + 2), (1, gb + 32 + 6)]
    return [(c, off + r) for c, r in rows]


def _init_canon_rows(off):
    """Rows of the canonical state cells as half-round 0 starts (the initial work vector, all in
    the init region; b2f_layout.h canon_state at hr = 0): the dense (a_1) and spread (a_2) limbs
    of h_0..h_7 (v_0..v_7), of the IV constants v_8..v_11 and v_15, and of the XOR results
    v_12..v_14 (even rows)."""
    rows = [4 * w + k for w in range(8) for k in range(4)]
    rows += [108 + 4 * i + k for i in (0, 1, 2, 3, 7) for k in range(4)]
    rows += [140 + 8 * a + 2 * k for a in range(3) for k in range(4)]
    return [(c, off + r) for r in rows for c in (1, 2)]


@pytest.mark.parametrize("rounds_choices,n,seed", [((12,), 600, 41), ((1, 4, 12, 13), 700, 42),
                                                   ((2, 3), 900, 43)])
def test_fast_pass_clean_and_carried_faults(engine, orc, rounds_choices, n, seed):
    import b2f

    x = random_inputs(n, rounds_choices, seed)
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    engine.sync(0)
    adv, fixed = batch.host_trace()
    adv, fixed = adv.copy(), fixed.copy()
    off = batch.offsets_host.astype(np.uint64)
    path, rep = _dev_eval(engine, batch, adv, fixed)
    assert path == 0, "the fast pass flagged a clean trace"
    assert rep["first_failure"] == NONE and rep["rows_checked"] == int(off[-1])
    rng = np.random.default_rng(seed)
    # canonical cells of half-rounds inside bands (carried) and at band starts (gathered): the
    # tiles of instance i are numbered from sum(2 rounds) over earlier instances
    insts = rng.choice(n, 6, replace=False)
    for i in insts:
        r_i = int((off[i + 1] - off[i] - 228) // ROUND_ROWS)
        if r_i < 1:
            continue
        for hr in sorted({1, 2, int(rng.integers(1, 2 * r_i + 1)), 2 * r_i}):
            cells = _canon_rows(int(off[i]), r_i, hr)
            c, r = cells[int(rng.integers(0, len(cells)))]
            a2 = adv.copy()
            a2[c, r] ^= np.uint32(1 << int(rng.integers(0, 16)))
            path, g = _dev_eval(engine, batch, a2, fixed)
            o = orc.evaluate(a2, fixed, off)
            assert g == o, (i, hr, c, r)
            if o["first_failure"] != NONE:
                assert path == 1, "a corruption the oracle sees was not handed to the exact kernel"
    # the batch restored: clean again, fast pass only
    path, rep = _dev_eval(engine, batch, adv, fixed)
    assert path == 0 and rep["first_failure"] == NONE


def test_fast_pass_tile_map_across_zero_round_runs(engine, orc):
    """The fast pass's tile descriptors (eval_desc_kernel: a wave searches the row map for its
    first tile, its lanes then search the next 64 instances and fall back to their own search
    past them) on a batch with runs of 0-round instances -- which own no half-round tile -- of
    1, 63, 64, 65 and 300 instances between 1-, 2- and 12-round ones: clean, then a fault in a
    half-round cell of the instance right after each run is handed to the exact kernel and
    reported where the oracle reports it."""
    import b2f

    x = random_inputs(1200, (1, 2, 12), 44)
    runs = [(10, 1), (40, 63), (200, 64), (400, 65), (700, 300)]
    for a, k in runs:
        x["rounds"][a:a + k] = 0
    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    engine.sync(0)
    adv, fixed = batch.host_trace()
    adv, fixed = adv.copy(), fixed.copy()
    off = batch.offsets_host.astype(np.uint64)
    path, rep = _dev_eval(engine, batch, adv, fixed)
    assert path == 0 and rep["first_failure"] == NONE and rep["rows_checked"] == int(off[-1])
    for a, k in runs:
        i = a + k  # the first instance after the run
        r = int(off[i]) + INIT_ROWS + 30  # a cell of its first half-round tile
        a2 = adv.copy()
        a2[4, r] ^= np.uint32(1 << 3)
        path, g = _dev_eval(engine, batch, a2, fixed)
        o = orc.evaluate(a2, fixed, off)
        assert o["first_failure"] != NONE and g == o and path == 1, (a, k)


EV_BAND = 24  # B2F_EVAL_HR_BAND: consecutive half-round tiles per wave visit (csrc/b2f_fused.hip)
PAD_ROWS = 256  # the edge walk's zero-row tiles: 64 quads


def _w_eval():
    """Upper bound on the fast pass's waves: 2 workgroups per CU x 4 waves (launch_eval_fast). A
    smaller grid only means more visits per wave."""
    import torch

    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


def _eval_now(engine, batch):
    batch.evaluate(engine)
    path = engine.debug_eval_path()
    return path, batch.report_dict()


def _check_flip(engine, batch, col, row, mask, want, what):
    """One device-side flip: the report equals `want()` (evaluated with the flip in place), a
    fault the oracle flags was handed to the exact kernel; the cell is restored. Returns whether
    the oracle flagged it."""
    dev_flip(batch, col, row, mask)
    try:
        path, g = _eval_now(engine, batch)
        o = want()
    finally:
        dev_flip(batch, col, row, mask)
    print("%s col %d row %d mask %#x: path %d, first_failure gpu %#x oracle %#x"
          % (what, col, row, mask, path, g["first_failure"], o["first_failure"]))
    assert g == o, (what, col, row, mask, g, o)
    if o["first_failure"] != NONE:
        assert path == 1, "a corruption the oracle sees was not handed to the exact kernel: %s" % (what,)
    return o["first_failure"] != NONE


@pytest.fixture(scope="module")
def edge_batch(engine, orc):
    """More than 2 W instances of 0 or 1 rounds and six zero-row tiles (the last one partial),
    filled on the device, with a host mirror of the clean trace: every wave of the fast pass walks
    instance tiles on a second and third visit (t += W), and the zero-row tiles land on waves
    that walked instance tiles before."""
    import b2f

    W = _w_eval()
    n = 2 * W + 37
    x = random_inputs(n, (0, 1), 61)
    used = int(b2f.offsets(x)[-1])
    total = used + 4 * (64 * 5 + 3)
    batch = b2f.DeviceBatch(x, total_rows=total)
    batch.advice.zero_()
    batch.fixed.zero_()
    batch.fill(engine)
    engine.sync(0)
    adv, fixed = batch.host_trace()
    adv, fixed = adv.copy(), fixed.copy()
    assert not adv[:, used:].any() and not fixed[used:].any()
    want = orc.evaluate(adv, fixed, batch.offsets_host)
    assert want["first_failure"] == NONE and want["rows_checked"] == total
    return W, n, used, total, batch, adv, fixed, want


def test_edge_walk_clean_batch_is_fast_pass_only(engine, orc, edge_batch):
    """The clean edge-walk batch costs the fast pass only (path == 0), and its report is the
    oracle's over total_rows.

    This batch first showed eval_desc_kernel reading the tiles before a tile's instance from a lane that
    had left the wave's shuffle (it read 0): with half the instances at 0 rounds a lane's instance
    lies further along the wave's 64 instances than its own tile, so tiles near the end of the
    batch, or in a wave with a lane past the 64, got half-round number = tile number, failed
    their copy checks and sent a correct trace to the exact kernel (a false alarm, never a false
    "clean")."""
    W, n, used, total, batch, adv, fixed, want = edge_batch
    path, rep = _eval_now(engine, batch)
    assert rep == want
    assert path == 0, "the fast pass flagged a clean trace"
    # a_5 of a zero row is constrained by nothing: clean on both sides, fast pass only
    r = used + 2 * PAD_ROWS + 9
    dev_flip(batch, 5, r, 1 << 7)
    try:
        path, g = _eval_now(engine, batch)
    finally:
        dev_flip(batch, 5, r, 1 << 7)
    adv[5, r] ^= np.uint32(1 << 7)
    try:
        o = orc.evaluate(adv, fixed, batch.offsets_host)
    finally:
        adv[5, r] ^= np.uint32(1 << 7)
    assert g == o and g["first_failure"] == NONE and path == 0


def test_edge_walk_faults_past_first_visit(engine, orc, edge_batch):
    """The eval's edge walk (eval_edge_walk: one tile per instance -- its init and final regions --
    then the zero rows as 64-quad tiles, dealt with stride W = waves of the launch) past a wave's
    first tile. Single cells are flipped on the device in the init and final regions of
    instances on both sides of the W and 2 W boundaries and in the zero rows; each report must
    equal the oracle's (a window of instances around the fault, re-based; the whole trace for the
    zero rows), and whatever the oracle flags must have reached the exact kernel. The restored
    trace is the clean one bit for bit and costs the fast pass only again."""
    import torch

    W, n, used, total, batch, adv, fixed, want = edge_batch
    off = batch.offsets_host
    rng = np.random.default_rng(61)
    insts = [0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, n - 1]
    insts += [int(i) for i in rng.choice(n, 4, replace=False)]
    cases = flagged = 0
    for i in insts:
        o_i = int(off[i])
        row_f = o_i + INIT_ROWS + ROUND_ROWS * rounds_of(off, i)
        for name, lo, hi in (("init", o_i, o_i + INIT_ROWS), ("final", row_f, row_f + 64)):
            cols = [0, 1, 2, FIXED_COL] + [int(c) for c in rng.integers(3, 10, 2)]
            for col in cols:
                r = int(rng.integers(lo, hi))
                hit = _check_flip(engine, batch, col, r, 1 << int(rng.integers(0, 16)),
                                  lambda: oracle_window(orc, batch, i), (name, i))
                if col in (0, 1, 2, FIXED_COL):
                    assert hit, ("the oracle does not flag this flip", name, i, col, r)
                flagged += hit
                cases += 1
    assert 3 * flagged >= 2 * cases, (flagged, cases)

    def whole(col, r, mask):
        def run():
            t = fixed if col == FIXED_COL else adv[col]
            t[r] ^= np.uint32(mask)
            try:
                return orc.evaluate(adv, fixed, off)
            finally:
                t[r] ^= np.uint32(mask)
        return run

    for r in (used, used + 255, used + 256, used + 3 * PAD_ROWS + 77, total - 5, total - 1):
        for col in (0, 1, 2, FIXED_COL):
            mask = 1 << int(rng.integers(0, 16))
            assert _check_flip(engine, batch, col, r, mask, whole(col, r, mask), ("pad", r - used)), \
                ("the oracle does not flag this flip", r - used, col)
    assert torch.equal(batch.advice.cpu(), torch.from_numpy(adv.view(np.int32)))
    assert torch.equal(batch.fixed.cpu(), torch.from_numpy(fixed.view(np.int32)))
    path, rep = _eval_now(engine, batch)
    assert path == 0 and rep == want, "the restored batch is not clean, or not by the fast pass alone"


def test_band_second_visit_faults(engine, orc):
    """The half-round pass's band loop past a wave's first band: more than 1.25 x 24 x W
    half-round tiles (rounds 12 and 5 mixed, so bands cross instances), i.e. a quarter of the
    waves jump to a band W bands further (bn = b + W) with the limb table carried from the tile
    before the jump in their staging, the last band is partial (tn >= n_hr inside a band) and band
    starts lie inside instances (the jn == 0 gather). Faults in the canonical cells a tile reads
    (carried or gathered: _canon_rows of its half-round, the init region's state cells for an
    instance's first half-round) and in those it holds (of the next half-round), for the first, a middle and the last tile of the first second-visit band, the
    next band's first tile, the last full band, the partial last band, the last tile, and an
    instance whose first half-round starts mid-band in a second-visit band."""
    import b2f
    W = _w_eval()
    need = (5 * EV_BAND * W + 3) // 4  # 1.25 x 24 x W
    n = (need * 103) // (17 * 100) + 8  # 17 tiles per instance on average, 3 % over
    for seed in range(51, 67):
        x = random_inputs(n, (12, 5), seed)
        cum = np.concatenate([[0], np.cumsum(2 * x["rounds"].astype(np.int64))])
        n_hr = int(cum[-1])
        starts = np.arange(EV_BAND * W, n_hr, EV_BAND)  # second-visit band starts
        inside = starts[~np.isin(starts, cum)]
        if n_hr >= need and n_hr % EV_BAND != 0 and inside.size:
            break
    assert n_hr >= need and n_hr % EV_BAND != 0 and inside.size, (n, n_hr, need)

    batch = b2f.DeviceBatch(x)
    batch.fill(engine)
    engine.sync(0)
    off = batch.offsets_host
    assert (int(off[-1]) - 228 * n) // 208 == n_hr
    path, rep = _eval_now(engine, batch)
    assert path == 0, "the fast pass flagged a clean trace"
    assert rep["first_failure"] == NONE and rep["rows_checked"] == int(off[-1])

    def inst_of(T):
        i = int(np.searchsorted(cum, T, side="right")) - 1
        return i, int(T - cum[i])

    last_full = (n_hr // EV_BAND - 1) * EV_BAND
    part = (n_hr // EV_BAND) * EV_BAND
    mid_start = [int(c) for c in cum[:-1] if c > EV_BAND * W and c % EV_BAND not in (0, EV_BAND - 1)]
    assert mid_start, "no instance starts mid-band in a second-visit band"
    tiles = {"band W first": EV_BAND * W, "band W middle": EV_BAND * W + 11,
             "band W last": EV_BAND * W + EV_BAND - 1, "band W+1 first": EV_BAND * (W + 1),
             "last full band first": last_full, "last full band last": last_full + EV_BAND - 1,
             "partial band first": part, "last tile": n_hr - 1,
             "instance start mid-band": mid_start[len(mid_start) // 2]}
    assert inst_of(int(inside[0]))[1] != 0
    tiles["band start inside an instance"] = int(inside[0])
    rng = np.random.default_rng(seed)
    for what, T in tiles.items():
        assert EV_BAND * W <= T < n_hr, (what, T)
        i, hr = inst_of(T)
        r_i = int(x["rounds"][i])
        picks = [("held", _canon_rows(int(off[i]), r_i, hr + 1))]  # rows of tile T itself
        if hr >= 1:
            picks.append(("read", _canon_rows(int(off[i]), r_i, hr)))  # rows of tile T - 1
        else:  # an instance's first half-round: its limb table is gathered from the init region
            picks.append(("read", _init_canon_rows(int(off[i]))))
        for kind, cells in picks:
            c, r = cells[int(rng.integers(0, len(cells)))]
            hit = _check_flip(engine, batch, c, r, 1 << int(rng.integers(0, 16)),
                              lambda: oracle_window(orc, batch, i), (what, kind, T, i, hr))
            assert hit, ("the oracle does not flag this flip", what, kind, c, r)
    path, rep = _eval_now(engine, batch)
    assert path == 0 and rep["first_failure"] == NONE, "the restored batch is not clean"
