"""b2f_msm_cells_dev on a caller-owned, non-blocking stream, queued behind in-flight work
(tests/test_gpu_side_stream.py's pattern: a cold run, then the same sequence behind a filler with no
host synchronisation). The call stages the host descriptors in pinned memory and uploads them on
the stream, so the sequence is the one that would expose a staging block rewritten too early:

  the first call, with a tail (its scalar multiplications fork to the context's side stream);
  its descriptor array overwritten with garbage by the host as soon as the call returns;
  a second call with other descriptors, another length and no tail queued straight behind it;
  a third with a tail again; one synchronise; all three results right.

Needs an MI355X (`-m gpu`)."""
import ctypes
import random

import numpy as np
import pytest

import cells_ref as cr
import msm_ref as mr

from test_gpu_side_stream import _cold_then_queued, _host, _same

pytestmark = pytest.mark.gpu

FORM, LEN_A, LEN_B, TAIL = 1, 3000, 1777, 6


def _prepare(eng, run):
    import torch

    cv = mr.curve_of_form(FORM)
    r = mr.ORDER[cv]
    rng = random.Random(1800 + run)
    bs, pts = mr.known_bases(FORM, LEN_A + TAIL)
    cells = np.array([rng.randrange(1 << 32) for _ in range(4 * LEN_A + 9)], dtype=np.uint32)
    cols_a = [(1, LEN_A, 0, 32), (LEN_A + 2, LEN_A - 5, 0, 16), (2 * LEN_A + 3, LEN_A, 16, 16), (5, LEN_A, 7, 1)]
    cols_b = [(3 * LEN_A, LEN_B, 3, 17), (7, LEN_B + 100, 0, 32)]
    tails = {}
    for name, n in (("a", len(cols_a)), ("c", len(cols_b))):
        tails[name] = [[rng.randrange(r) for _ in range(TAIL)] for _ in range(n)]

    def want(cols, ln, tail):
        return mr.pack_points(cv, [mr.expected_msm(FORM, cr.column_scalars(cells, col, ln) + (tail[j] if tail else []),
                                                   bs[:ln] + (bs[ln:ln + TAIL] if tail else []))
                                   for j, col in enumerate(cols)])

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")  # noqa: E731
    return dict(cells=torch.from_numpy(cells.view(np.int32)).to("cuda:0"), bases=dev(mr.pack_points(cv, pts)),
                cols_a=cols_a, cols_b=cols_b,
                tail_a=dev(np.stack([mr.pack_scalars(FORM, t) for t in tails["a"]])),
                tail_c=dev(np.stack([mr.pack_scalars(FORM, t) for t in tails["c"]])),
                want=[want(cols_a, LEN_A, tails["a"]), want(cols_b, LEN_B, None), want(cols_b, LEN_B, tails["c"])])


def _issue(eng, data, mark):
    import torch

    from b2f import _lib

    s = torch.cuda.current_stream().cuda_stream
    cells, bases = data["cells"], data["bases"]
    outs = [torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0") for n in (4, 2, 2)]

    def call(cols, ln, tail, out):
        arr = _lib.cell_columns(cols)  # built for this call alone, and dropped after it
        eng.msm_cells_dev(cells.data_ptr(), cells.numel(), arr, ln, tail.data_ptr() if tail is not None else 0,
                          TAIL if tail is not None else 0, bases.data_ptr(), bases.shape[0], FORM, out.data_ptr(), s)
        ctypes.memset(arr, 0xff, ctypes.sizeof(arr))  # the host array is the caller's again

    call(data["cols_a"], LEN_A, data["tail_a"], outs[0])
    if mark():
        return None
    call(data["cols_b"], LEN_B, None, outs[1])
    call(data["cols_b"], LEN_B, data["tail_c"], outs[2])
    return outs


def _check(data, outs):
    for i, (out, want) in enumerate(zip(outs, data["want"])):
        _same(_host(out), want, ("cell commitments of call", i))


def test_cell_commitments_queue_behind_in_flight_work_and_copy_their_descriptors():
    _cold_then_queued("msmcells", _prepare, _issue, _check)
