"""b2f_msm_cells_dev against what a caller had to do before it for the same points: b2f_export_fp_dev
into a block of field elements, then b2f_msm_dev on the block. Both curves, a real trace (a filled
batch of 12-round instances), HIP-event times on the stream, the two paths interleaved rep by rep
in one process, medians and min-max of --reps. One JSON line per row, appended to
profiles/msm_cells_bench.jsonl, each with the source stamp.

Default rows: len = 2^17 and 2^20 with 1 and 10 columns (one circuit), and 64 circuits x 10 columns
at 2^17. `faster_beyond_spread`: the parent path's median exceeds the new call's by more than the
two paths' min-max spreads together; stated with the export counted and without it. The parent path
exports all ten columns of a circuit whatever it commits to (the export has no narrower form).
--sweep 8,9,..: the forced window width (diagnostics library, B2F_DIAG_MSM_PLAN) for ten columns of
  16-bit and of 32-bit fields of the same cells at every length: the lines msm_cells_default_window
  (b2f_msm.hip) is checked against.
--tail N: ten columns at 2^17 with no tail against a tail of N rows, interleaved, and on the diagnostics
  library the tail beside the cell passes against the tail on the call's own stream
  (B2F_DIAG_MSM_TAIL=serial).
The results of the two paths are compared bit for bit on the device before anything is timed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_quotient import _stats  # noqa: E402

BASE_POINTS = 1 << 15  # distinct bases, tiled to len: the cost of a call does not depend on them
INSTANCE_ROWS = 5220   # a 12-round instance


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", default="17,20", help="log2 of the lengths")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--circuits", type=int, default=64, help="circuits of the batched row (0: skip it)")
    ap.add_argument("--sweep", default="", help="window widths to force, e.g. 8,9,10,11,12,13,14,15,16")
    ap.add_argument("--tail", type=int, default=0, help="tail rows of the tail A/B (0: skip it)")
    ap.add_argument("--no-rows", action="store_true", help="skip the rows against the parent path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_cells_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import b2f
    import msm_ref as mr
    from b2f import _lib, synth

    sweep = [int(v) for v in args.sweep.split(",") if v]
    eng = b2f.Engine(0)
    diag = b2f.Engine(0, diag=True) if sweep or args.tail else None
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    lens = [1 << int(v) for v in args.lens.split(",")]
    rows_needed = max(max(lens), (args.circuits << 17) if args.circuits and not args.no_rows else 0)
    batch = b2f.DeviceBatch(synth.batch(rows_needed // INSTANCE_ROWS + 1, rounds_mix=[12]), device="cuda:0")
    batch.fill_evaluate(eng)
    eng.sync(s)
    total = batch.total_rows
    assert total >= rows_needed
    lines = []

    def emit(rec):
        rec = dict({"stamp": _lib.source_stamp()}, **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(*fns):
        """Device ms of each of fns, run back to back on the stream (events between them)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        ev[0].record(stream)
        for i, fn in enumerate(fns):
            fn()
            ev[i + 1].record(stream)
        ev[-1].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(fns))]

    def spread(st):
        return st["max"] - st["min"]

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        cv = mr.curve_of_form(form)
        curve = "bn254_g1" if cv else "vesta"
        _, pts = mr.known_bases(form, BASE_POINTS, incremental=True)
        base = torch.from_numpy(mr.pack_points(cv, pts).view(np.int64)).to("cuda:0")
        bases = base.repeat(max(lens) // BASE_POINTS + 2, 1).contiguous()
        cases = [] if args.no_rows else [(ln, 1, n) for ln in lens for n in (1, 10)]
        if args.circuits and not args.no_rows:
            cases.append((1 << 17, args.circuits, 10))
        for ln, circuits, per in cases:
            begins = [c * ln for c in range(circuits)]
            cols = []
            for b in begins:
                cols += b2f.advice_cell_columns(total, b, ln)[:per]
            arr = _lib.cell_columns(cols)
            n_cols = len(cols)
            block = torch.empty((10 * circuits, ln, 4), dtype=torch.int64, device="cuda:0")
            out_new = torch.empty((n_cols, 8), dtype=torch.int64, device="cuda:0")
            out_old = torch.empty((10 * circuits, 8), dtype=torch.int64, device="cuda:0")

            def new():
                eng.msm_cells_dev(batch.advice.data_ptr(), batch.advice.numel(), arr, ln, 0, 0, bases.data_ptr(),
                                  ln, form, out_new.data_ptr(), s)

            def export():
                for c, b in enumerate(begins):
                    eng.export_fp_dev(batch.advice.data_ptr(), total, b, ln, form,
                                      block[10 * c:10 * c + 10].data_ptr(), ln, s)

            def old_msm():
                # the first `per` columns of each circuit: one call per circuit unless all ten are taken
                if per == 10:
                    eng.msm_dev(block.data_ptr(), ln, ln, n_cols, bases.data_ptr(), ln, form, out_old.data_ptr(), s)
                else:
                    for c in range(circuits):
                        eng.msm_dev(block[10 * c:].data_ptr(), ln, ln, per, bases.data_ptr(), ln, form,
                                    out_old[per * c:].data_ptr(), s)

            timed(new, export, old_msm)  # warm: grows the scratch
            assert torch.equal(out_new, out_old[:n_cols]), "the two paths disagree"
            t = [[], [], []]
            for _ in range(args.reps):
                for i, ms in enumerate(timed(new, export, old_msm)):
                    t[i].append(ms)
            st_new, st_exp, st_msm = _stats(t[0]), _stats(t[1]), _stats(t[2])
            st_tot = _stats([a + b for a, b in zip(t[1], t[2])])
            emit({"what": "cells_vs_export_msm", "curve": curve, "len": ln, "circuits": circuits, "n_cols": n_cols,
                  "reps": args.reps, "plan": _lib.msm_cells_plan(cols, ln, form=form), "new_ms": st_new,
                  "parent_export_ms": st_exp, "parent_msm_ms": st_msm, "parent_total_ms": st_tot,
                  "ratio_with_export": round(st_tot["median"] / st_new["median"], 3),
                  "ratio_without_export": round(st_msm["median"] / st_new["median"], 3),
                  "faster_beyond_spread_with_export":
                      st_tot["median"] - st_new["median"] > spread(st_tot) + spread(st_new),
                  "faster_beyond_spread_without_export":
                      st_msm["median"] - st_new["median"] > spread(st_msm) + spread(st_new)})
            del block
        if args.tail:
            ln = 1 << 17
            cols = b2f.advice_cell_columns(total, 0, ln)
            arr = _lib.cell_columns(cols)
            tail = torch.randint(-2**63, 2**63 - 1, (10, args.tail, 4), dtype=torch.int64, device="cuda:0")
            tail[:, :, 3] &= 2**60 - 1  # 252-bit values: below both moduli, used as Montgomery residues
            out = torch.empty((10, 8), dtype=torch.int64, device="cuda:0")

            def with_tail(rows, e=eng, serial=False):
                if serial:
                    os.environ["B2F_DIAG_MSM_TAIL"] = "serial"
                try:
                    e.msm_cells_dev(batch.advice.data_ptr(), batch.advice.numel(), arr, ln, tail.data_ptr() if rows else 0,
                                    rows, bases.data_ptr(), ln + rows, form, out.data_ptr(), s)
                finally:
                    os.environ.pop("B2F_DIAG_MSM_TAIL", None)

            # no tail, the tail beside the cell passes (product), and on the diagnostics library the
            # same against the tail on the call's own stream
            variants = [lambda: with_tail(0), lambda: with_tail(args.tail), lambda: with_tail(args.tail, diag),
                        lambda: with_tail(args.tail, diag, True)]
            timed(*variants)
            t = [[] for _ in variants]
            for _ in range(args.reps):
                for i, ms in enumerate(timed(*variants)):
                    t[i].append(ms)
            emit({"what": "tail_ab", "curve": curve, "len": ln, "n_cols": 10, "tail_rows": args.tail, "reps": args.reps,
                  "no_tail_ms": _stats(t[0]), "tail_ms": _stats(t[1]), "diag_tail_overlapped_ms": _stats(t[2]),
                  "diag_tail_serial_ms": _stats(t[3])})
        for ln in lens if sweep else []:
            for bits in (16, 32):
                cols = [(o, a, 0, bits) for o, a, _, _ in b2f.advice_cell_columns(total, 0, ln)]
                arr = _lib.cell_columns(cols)
                out = torch.empty((10, 8), dtype=torch.int64, device="cuda:0")

                def forced():
                    diag.msm_cells_dev(batch.advice.data_ptr(), batch.advice.numel(), arr, ln, 0, 0, bases.data_ptr(),
                                       ln, form, out.data_ptr(), s)

                default_c = _lib.msm_cells_plan(cols, ln, form=form)["window_bits"]
                t = {c: [] for c in sweep}
                try:
                    for rep in range(args.reps + 1):  # widths interleaved rep by rep; the first rep warms
                        for c in sweep:
                            os.environ["B2F_DIAG_MSM_PLAN"] = str(c)
                            ms = timed(forced)[0]
                            if rep:
                                t[c].append(ms)
                finally:
                    os.environ.pop("B2F_DIAG_MSM_PLAN", None)
                best = min(sweep, key=lambda c: _stats(t[c])["median"])
                for c in sweep:
                    st = _stats(t[c])
                    emit({"what": "window_sweep", "curve": curve, "len": ln, "n_cols": 10, "bits": bits, "forced_c": c,
                          "default_c": default_c, "reps": args.reps, "ms": st,
                          "over_best": round(st["median"] / _stats(t[best])["median"], 4)})
        del bases
    eng.close()
    if diag:
        diag.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
