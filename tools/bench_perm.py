"""Throughput of the permutation-argument prover columns: a circuit of 2^k rows filled with
12-round instances; the per-proof z call (b2f_permutation_columns_dev without sigma) and the
keygen sigma call (b2f_permutation_sigma_dev) timed with HIP events (b2f_kernel_times). One
JSON line per form.

--circuits C: C such circuits cut from one batch; the batch call
(b2f_permutation_columns_batch_dev) against the loop of C single calls, in this process, rep by
rep in turn. Per side the HIP-event time of the timed regions and the wall time from the first
call to the return of b2f_sync (the single calls' host setup is part of what a prover pays).
--ab LIB: the single call of this library against LIB's (a build of another revision,
tools/build_rev.sh), rep by rep in turn."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "zk-odst_amd"))


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def _timed(eng, s, fn):
    """(HIP-event ms of the perm regions, wall ms from the first call to the end of sync)."""
    eng.set_timing(True)
    t0 = time.perf_counter()
    fn()
    eng.sync(s)
    wall = (time.perf_counter() - t0) * 1e3
    return eng.kernel_times()["perm"][0], wall


def bench_circuits(args, eng, torch, b2f, synth):
    """One JSON line per form: batch call vs the loop of single calls."""
    from b2f import _lib

    C = args.circuits
    n_rows = 1 << args.k
    usable = n_rows - 7
    # 12-round instances, or below k = 13 (where none fits) one instance of as many rounds as fit
    rounds = 12 if usable >= 5220 else (usable - 228) // 416
    per = usable // (228 + 416 * rounds)
    batch = b2f.DeviceBatch(synth.batch(per * C, rounds=rounds))
    batch.fill(eng)
    s = torch.cuda.current_stream().cuda_stream
    eng.sync(s)
    first = [per * c for c in range(C + 1)]
    sets = (8 + args.chunk - 1) // args.chunk
    dev = batch.advice.device
    from b2f import field

    for form in [int(f) for f in args.forms.split(",")]:
        f = field.of_form(form)
        w, d = field.omega(f, args.k), field.delta(f)
        zb = torch.empty((C, sets, n_rows, 4), dtype=torch.int64, device=dev)
        zs = torch.empty((C, sets, n_rows, 4), dtype=torch.int64, device=dev)
        adv, total, off = batch.advice.data_ptr(), batch.total_rows, batch.offsets_host

        def run_batch():
            eng.permutation_columns_batch_dev(adv, total, off, first, args.k, usable, w, d, 3, 5,
                                              args.chunk, form, zb.data_ptr(), n_rows, s)

        def run_loop():
            for c in range(C):
                eng.permutation_columns_dev(adv, total, off[first[c]:first[c + 1] + 1], args.k, usable,
                                            w, d, 3, 5, args.chunk, form, 0, zs[c].data_ptr(), n_rows, s)

        run_batch()
        run_loop()
        eng.sync(s)
        equal = bool(torch.equal(zb[:, :, :usable + 1], zs[:, :, :usable + 1]))
        ev = {"batch": [], "loop": []}
        wall = {"batch": [], "loop": []}
        for _ in range(args.reps):
            for name, fn in (("batch", run_batch), ("loop", run_loop)):
                e, wl = _timed(eng, s, fn)
                ev[name].append(e)
                wall[name].append(wl)
        eng.set_timing(False)
        rows = C * n_rows
        print(json.dumps({
            "stamp": _lib.source_stamp(), "lib": args.lib or "product", "k": args.k, "circuits": C,
            "instances_per_circuit": per, "rounds": rounds, "form": form, "chunk_len": args.chunk,
            "reps": args.reps,
            "outputs_equal": equal,
            "batch_event_ms": _stats(ev["batch"]), "loop_event_ms": _stats(ev["loop"]),
            "batch_wall_ms": _stats(wall["batch"]), "loop_wall_ms": _stats(wall["loop"]),
            "batch_ns_per_row": round(_stats(ev["batch"])["median"] * 1e6 / rows, 4),
            "loop_ns_per_row": round(_stats(ev["loop"])["median"] * 1e6 / rows, 4)}), flush=True)
        del zb, zs


def bench_ab(args, eng, torch, b2f, synth):
    """One JSON line per form: this library's single call vs --ab's, interleaved."""
    from b2f import _lib

    other = b2f.Engine(0, lib_path=args.ab)
    n_rows = 1 << args.k
    usable = n_rows - 7
    batch = b2f.DeviceBatch(synth.batch(usable // 5220, rounds=12))
    batch.fill(eng)
    s = torch.cuda.current_stream().cuda_stream
    eng.sync(s)
    for form in [int(f) for f in args.forms.split(",")]:
        sides = (("this", eng), ("other", other))
        ev = {n: [] for n, _ in sides}
        wall = {n: [] for n, _ in sides}
        for rep in range(args.reps + 1):  # rep 0 warms both contexts up
            for name, e in sides:
                z = []
                t, wl = _timed(e, s, lambda: z.append(batch.permutation_columns(
                    e, args.k, usable, 3, 5, chunk_len=args.chunk, form=form, sigma=False)[1]))
                if rep:
                    ev[name].append(t)
                    wall[name].append(wl)
                del z
        print(json.dumps({
            "stamp": _lib.source_stamp(), "this": args.lib or "product", "other": args.ab, "k": args.k,
            "form": form, "chunk_len": args.chunk, "reps": args.reps,
            "this_event_ms": _stats(ev["this"]), "other_event_ms": _stats(ev["other"]),
            "this_wall_ms": _stats(wall["this"]), "other_wall_ms": _stats(wall["other"]),
            "this_ns_per_row": round(_stats(ev["this"])["median"] * 1e6 / n_rows, 4)}), flush=True)
    other.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=22)
    ap.add_argument("--chunk", type=int, default=3)
    ap.add_argument("--forms", default="1,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="a variant library (A/B), default the product")
    ap.add_argument("--circuits", type=int, default=0,
                    help="C circuits of 2^k rows: the batch call vs the loop of C single calls")
    ap.add_argument("--ab", default=None, help="another build's library: single call A/B, interleaved")
    args = ap.parse_args()
    import torch

    import b2f
    from b2f import synth

    eng = b2f.Engine(0) if not args.lib else b2f.Engine(0, lib_path=args.lib)
    if args.circuits:
        return bench_circuits(args, eng, torch, b2f, synth)
    if args.ab:
        return bench_ab(args, eng, torch, b2f, synth)
    n_rows = 1 << args.k
    usable = n_rows - 7
    n_inst = usable // 5220
    batch = b2f.DeviceBatch(synth.batch(n_inst, rounds=12))
    batch.fill(eng)
    s = torch.cuda.current_stream().cuda_stream
    eng.sync(s)
    for form in [int(f) for f in args.forms.split(",")]:
        batch.permutation_columns(eng, args.k, usable, 3, 5, chunk_len=args.chunk, form=form, sigma=False)
        sig = batch.permutation_sigma(eng, args.k, form=form)
        eng.sync(s)
        eng.set_timing(True)
        for _ in range(args.reps):
            _, z = batch.permutation_columns(eng, args.k, usable, 3, 5, chunk_len=args.chunk,
                                             form=form, sigma=False)
            sig = batch.permutation_sigma(eng, args.k, form=form)
        eng.sync(s)
        kt = eng.kernel_times()
        ms, cnt = kt["perm"]
        sms, scnt = kt["perm_sigma"]
        per, sper = ms / cnt, sms / scnt
        sets = (8 + args.chunk - 1) // args.chunk
        print(json.dumps({"lib": args.lib or "product", "k": args.k, "instances": n_inst, "form": form,
                          "chunk_len": args.chunk, "z_ms_per_call": round(per, 3),
                          "sigma_ms_per_call": round(sper, 3), "rows_per_s": round(n_rows / per * 1e3),
                          "z_written_GBps": round(usable * 32 * sets / per / 1e6, 1)}))
        del sig, z


if __name__ == "__main__":
    main()
