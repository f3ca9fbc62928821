"""The pass kernel of b2f_ntt_columns_dev under pass plans the product picks only at sizes no test
can check row by row: three passes (k = 17..24) and four (k = 25..28). The diagnostics library
reads B2F_DIAG_NTT_PLAN=l1,l2[,l3[,l4]] at the call and runs those digits instead of ntt_plan's,
so the same code (the load and store index maps over two and three remaining digits, nat_to_sto /
sto_to_nat, the inter-pass twiddles, the in-place later passes) runs at k = 11..16, where
tests/ntt_ref.py gives every row.

  1  three- and four-pass plans at k = 11..16, every row against the reference: both directions,
     all four forms, a random shift and shift 1, a dense and a {0, 1, p-1} column, padded column
     strides with the output pattern intact past n, in_len in {n, n/4, 1} with garbage past it.
     The four-pass plans are the four shapes of k = 25..28 (zero to three leading digits one
     wider than the rest);
  2  four passes with the product's digit widths (5 and 6) at k = 20..23: bit for bit the
     product's own three-pass output of the same call, whose index path shares nothing with it
     past pass 1; k = 21 also against the sparse six-term direct sum;
  3  a malformed plan is refused with B2F_ERR_ARG, nothing launched, never run and never
     replaced silently.

Needs an MI355X (`-m gpu`)."""
import contextlib
import os

import numpy as np
import pytest

import ntt_ref as nr

pytestmark = pytest.mark.gpu

FWD, INV = 0, 1
ERR_ARG = 1
VAR = "B2F_DIAG_NTT_PLAN"

THREE = [(4, 4, 3), (5, 4, 4), (5, 5, 5), (6, 5, 5)]
FOUR = [(3, 3, 3, 2), (3, 3, 3, 3), (4, 3, 3, 3), (4, 4, 3, 3), (4, 4, 4, 3), (4, 4, 4, 4)]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _omega(form, k):
    from b2f import field

    return field.omega(field.of_form(form), k)


def _pattern(shape):
    return np.full(shape, 0xA5A5A5A5DEADBEEF, dtype=np.uint64)


def _first_diff(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return int(bad[0]) if len(bad) else None


@contextlib.contextmanager
def _forced(plan, k):
    """The plan in force for the calls inside, and shown to be (b2f_debug_ntt_plan)."""
    from b2f import _lib

    os.environ[VAR] = ",".join(str(d) for d in plan)
    try:
        assert _lib.debug_ntt_plan(k) == list(plan)
        yield
    finally:
        os.environ.pop(VAR, None)
    assert _lib.debug_ntt_plan(k) != list(plan)


def _run(engine, x, in_len, k, direction, shift, form, out_rows):
    d_in = _dev(x)
    d_out = _dev(_pattern((x.shape[0], out_rows, 4)))
    engine.ntt_columns_dev(d_in.data_ptr(), x.shape[1], in_len, x.shape[0], k, _omega(form, k), shift,
                           direction, form, d_out.data_ptr(), out_rows, _stream())
    engine.sync(_stream())
    return _host(d_out)


# ---------------------------------------------------------------------------------------------
# 1. every row


@pytest.mark.parametrize("plan", THREE + FOUR, ids=lambda p: "-".join(map(str, p)))
def test_forced_plan_every_row(diag_engine, plan):
    k = sum(plan)
    n = 1 << k
    idx = (THREE + FOUR).index(plan)
    rng = np.random.default_rng(700 + idx)
    in_rows, out_rows = n + 3, n + 5
    field_f, field_i = idx % 2, 1 - idx % 2  # forward runs in one field, inverse runs in the other
    # (direction, shift is random, in_len, form): the four forms in every plan
    runs = [(FWD, True, n, 2 * field_f), (FWD, False, n // 4, 2 * field_f + 1), (FWD, True, 1, 2 * field_f),
            (INV, True, n, 2 * field_i + 1), (INV, False, n, 2 * field_i)]
    assert {r[3] for r in runs} == {0, 1, 2, 3}
    cols, inv1 = {}, {}
    for fld in (0, 1):
        p = nr.modulus(2 * fld)
        dense = nr.random_elements(rng, in_rows, p)  # rows >= in_len: garbage that must not count
        special = [(0, 1, p - 1)[v] for v in rng.integers(0, 3, in_rows)]
        special[0] = p - 1
        cols[fld] = [dense, special]
        assert all(v != 0 for v in dense)
    with _forced(plan, k):
        for direction, rand_shift, in_len, form in runs:
            p = nr.modulus(form)
            fld = form >> 1
            shift = 2 + nr.random_elements(rng, 1, p - 2)[0] if rand_shift else 1
            x = np.stack([nr.pack(c, form) for c in cols[fld]])
            got = _run(diag_engine, x, in_len, k, direction, shift, form, out_rows)
            w = _omega(form, k)
            for c, vals in enumerate(cols[fld]):
                if direction == FWD and in_len == 1:
                    want = [vals[0]] * n  # sum_j x[j] (shift w^i)^j with the one term j = 0
                elif direction == FWD:
                    want = nr.forward(vals[:in_len], k, w, shift, p)
                else:
                    # out[j] = shift^-j n^-1 sum_i x[i] w^(-i j): the shift-1 reference, computed
                    # once per column, then row j times shift^-j
                    if (fld, c) not in inv1:
                        inv1[(fld, c)] = nr.inverse(vals[:n], k, w, 1, p)
                    si, s, want = pow(shift, -1, p), 1, []
                    for v in inv1[(fld, c)]:
                        want.append(v * s % p)
                        s = s * si % p
                bad = _first_diff(got[c, :n], nr.pack(want, form))
                assert bad is None, (plan, direction, in_len, form, c, "row %s" % bad)
                assert (got[c, n:] == _pattern((out_rows - n, 4))).all(), (plan, direction, form, c)


# ---------------------------------------------------------------------------------------------
# 2. the product's digit widths in four passes


def _random_device(n_cols, rows, seed):
    import torch

    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    shape = (n_cols, rows, 4)
    x = torch.randint(0, 2**32, shape, dtype=torch.int64, device="cuda:0", generator=g) << 32
    x |= torch.randint(0, 2**32, shape, dtype=torch.int64, device="cuda:0", generator=g)
    x[:, :, 3] &= (1 << 61) - 1  # < 2^253: an element of either field in any form
    return x


@pytest.mark.parametrize("plan", [(5, 5, 5, 5), (6, 5, 5, 5), (6, 6, 5, 5), (6, 6, 6, 5)],
                         ids=lambda p: "-".join(map(str, p)))
def test_four_passes_equal_the_product_three(diag_engine, plan):
    import torch

    from b2f import _lib

    k = sum(plan)
    n = 1 << k
    form = 1 if k % 2 else 3
    p = nr.modulus(form)
    rng = np.random.default_rng(800 + k)
    shift = 2 + nr.random_elements(rng, 1, p - 2)[0]
    assert len(_lib.debug_ntt_plan(k)) == 3
    x = _random_device(1, n, 8000 + k)
    fwd3 = diag_engine.ntt_columns(x, k, shift=shift, form=form)
    inv3 = diag_engine.ntt_columns(x, k, inverse=True, shift=shift, form=form)
    diag_engine.sync(_stream())
    with _forced(plan, k):
        fwd4 = diag_engine.ntt_columns(x, k, shift=shift, form=form)
        inv4 = diag_engine.ntt_columns(x, k, inverse=True, shift=shift, form=form)
        diag_engine.sync(_stream())
    assert not torch.equal(fwd3, x) and not torch.equal(inv3, fwd3)
    assert torch.equal(fwd4, fwd3)
    assert torch.equal(inv4, inv3)
    if k != 21:
        return
    del fwd3, inv3, fwd4, inv4, x
    # the truth: a sparse input against its six-term direct sum (as test_gpu_ntt.test_pass_plans)
    w = _omega(form, k)
    pos = sorted({0, 1, (1 << 10) - 1, 1 << 10, n // 2 + 3, n - 1})
    coef = nr.random_elements(rng, len(pos), p)
    x = torch.zeros((1, n, 4), dtype=torch.int64, device="cuda:0")
    x[0, torch.tensor(pos, device="cuda:0")] = _dev(nr.pack(coef, form))
    with _forced(plan, k):
        out = diag_engine.ntt_columns(x, k, shift=shift, form=form)
        diag_engine.sync(_stream())
    rows = sorted({0, 1, n - 1} | set(int(r) for r in rng.integers(0, n, 4096)))
    got = _host(out[0, torch.tensor(rows, device="cuda:0")])
    want = []
    for i in rows:
        pt = shift * pow(w, i, p) % p
        want.append(sum(c * pow(pt, j, p) for j, c in zip(pos, coef)) % p)
    bad = _first_diff(got, nr.pack(want, form))
    assert bad is None, "row %d" % rows[bad]


# ---------------------------------------------------------------------------------------------
# 3. malformed plans


@pytest.mark.parametrize("value,k", [("6,6", 11), ("4,4,4", 11),          # the sum is not k
                                     ("0,8,3", 11), ("9,2", 11),          # a digit 0 or 9
                                     ("3,2,2,2,2", 11),                   # five digits
                                     ("5,5", 10), ("8", 8),               # k <= 10: one pass, no plan
                                     ("", 11), ("6,5,", 11), ("11", 11), ("6;5", 11)])
def test_malformed_plan_is_refused_then_a_clean_call_is_right(diag_engine, value, k):
    from b2f import B2FError

    form = 1
    p = nr.modulus(form)
    n = 1 << k
    rng = np.random.default_rng(900 + k)
    vals = nr.random_elements(rng, n, p)
    x = nr.pack(vals, form)[None]
    d_in = _dev(x)
    d_out = _dev(_pattern((1, n, 4)))
    args = (d_in.data_ptr(), n, n, 1, k, _omega(form, k), 3, FWD, form, d_out.data_ptr(), n, _stream())
    os.environ[VAR] = value
    try:
        with pytest.raises(B2FError) as e:
            diag_engine.ntt_columns_dev(*args)
        assert e.value.code == ERR_ARG
    finally:
        os.environ.pop(VAR, None)
    diag_engine.sync(_stream())
    assert (_host(d_out) == _pattern((1, n, 4))).all()  # nothing was launched
    diag_engine.ntt_columns_dev(*args)
    diag_engine.sync(_stream())
    want = nr.pack(nr.forward(vals, k, _omega(form, k), 3, p), form)
    assert _first_diff(_host(d_out)[0], want) is None
