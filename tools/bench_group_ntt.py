"""Times of the group NTT (b2f_group_ntt_dev, inverse direction: g -> g_lagrange): both curves,
HIP-event times (b2f_kernel_times) of whole calls, medians over --reps calls after a warm-up call.
JSON lines appended to profiles/group_ntt_bench.jsonl, each with the source stamp and `run` (the
label given with --run).

  kind = "group_ntt"  one case (curve, k): the call's median, the scalar multiplications it performs
                      (b2f_group_ntt_plan) and the model = scalar_muls * t_sm, where t_sm is measured
                      in the same process, interleaved with the calls: b2f_ipa_fold_dev at len = 2^21
                      collapses 2^20 points, each one uniform-scalar multiplication on the same curve
                      arithmetic (plus a mixed addition and an affine conversion), so t_sm = t_fold /
                      2^20. ratio = time / model; the target at k = 20 is <= 1.35, the cost of a fully
                      divergent per-lane double-and-add over a uniform one. identity_outputs counts
                      all-zero points of the result: a degenerate input (whose intermediate points
                      are identities, which multiply for free) would show there.
  --stages CSV        no GPU: the per-stage times of one call from a rocprofv3 --kernel-trace CSV of a
                      separate run of this tool (--ks 20 --reps 1 --curves vesta): the launches of the
                      last call of the trace, in order, as one JSON line (kind = "stages").

The inputs are 4,096 known multiples of the generator laid out as i -> base[(i + s(i >> 12)) mod
4096], s(r) = 17 r + 5 r^2: tiling them plainly would make a periodic input, whose transform is
the identity almost everywhere."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_quotient import _stats  # noqa: E402

BASE_POINTS = 1 << 12
FOLD_LOG = 21


def stages(path, out, run):
    """The launches of the last group NTT in a kernel-trace CSV, in start order."""
    from b2f import _lib

    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "gntt_" not in name and "ipa_powers_kernel" not in name:
            continue
        short = name.split("(anonymous namespace)::", 1)[-1].split("(")[0]
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "gntt_root_check" in r[2]]
    call = rows[starts[-1]:]
    stage, launches = 1, []
    for t0, t1, name in call:
        rec = {"kernel": name, "ms": round((t1 - t0) / 1e6, 4)}
        if "gntt_first" in name or "gntt_stage" in name:
            rec["stage"] = stage
            stage += 1
        launches.append(rec)
    k = stage - 1
    rec = {"stamp": _lib.source_stamp(), "run": run, "kind": "stages", "k": k, "calls_in_trace": len(starts),
           "span_ms": round((call[-1][1] - call[0][0]) / 1e6, 4), "sum_ms": round(sum(r["ms"] for r in launches), 4),
           "launches": launches}
    line = json.dumps(rec)
    print(line)
    with open(out, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="12,16,20")
    ap.add_argument("--curves", default="vesta,bn254_g1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="unnamed")
    ap.add_argument("--stages", default="", help="a rocprofv3 kernel-trace CSV to summarise (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_ntt_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if args.stages:
        return stages(args.stages, args.out, args.run)
    import random

    import numpy as np
    import torch

    import b2f
    import msm_ref as mr
    from b2f import _lib, field

    ks = [int(v) for v in args.ks.split(",") if v]
    eng = b2f.Engine(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(rec):
        rec = dict({"stamp": _lib.source_stamp(), "run": args.run, "reps": args.reps}, **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(fn):
        eng.set_timing(True)
        fn()
        eng.sync(s)
        return eng.kernel_times()["quotient"][0]

    def spread(base, n):
        i = torch.arange(n, dtype=torch.int64, device="cuda:0")
        r = i >> 12
        return base[(i + 17 * r + 5 * r * r) % BASE_POINTS].contiguous()

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        cv = mr.curve_of_form(form)
        curve = "bn254_g1" if cv else "vesta"
        if curve not in args.curves.split(","):
            continue
        r = mr.ORDER[cv]
        rng = random.Random(9 + cv)
        _, pts = mr.known_bases(form, BASE_POINTS, incremental=True)
        base = torch.from_numpy(mr.pack_points(cv, pts).view(np.int64)).to("cuda:0")
        # the yardstick: one fold of 2^21, i.e. 2^20 uniform-scalar multiplications
        fn_ = 1 << FOLD_LOG
        fg0 = spread(base, fn_)
        fg = fg0.clone()
        fp = torch.randint(-2**63, 2**63 - 1, (fn_, 4), dtype=torch.int64, device="cuda:0")
        fp[:, 3] = (fp[:, 3] >> 3) & (2**61 - 1)  # 253-bit values are below both moduli
        fb = fp.clone()
        us = [rng.randrange(1, r) for _ in range(args.reps + 1)]

        def fold(rep):
            fg.copy_(fg0)
            return timed(lambda: eng.ipa_fold_dev(fp.data_ptr(), fb.data_ptr(), fg.data_ptr(), fn_, us[rep], form, s))

        for k in ks:
            n = 1 << k
            g = spread(base, n)
            out = torch.empty_like(g)
            omega = field.omega(field.of_form(form), k)
            t_call, t_fold = [], []
            for rep in range(args.reps + 1):  # the first pass warms both and grows the scratch
                tf = fold(rep)
                tc = timed(lambda: eng.group_ntt_dev(g.data_ptr(), k, omega, _lib.NTT_INVERSE, form, out.data_ptr(), s))
                if rep:
                    t_fold.append(tf)
                    t_call.append(tc)
            eng.set_timing(False)
            plan = _lib.group_ntt_plan(k, form)
            call, foldm = _stats(t_call), _stats(t_fold)
            t_sm = foldm["median"] / (fn_ // 2)
            model = plan["scalar_muls"] * t_sm
            emit({"kind": "group_ntt", "curve": curve, "k": k, "direction": "inverse", "call_ms": call,
                  "scalar_muls": plan["scalar_muls"], "scratch_bytes": plan["scratch_bytes"],
                  "fold_len": fn_, "fold_ms": foldm, "t_sm_ns": round(t_sm * 1e6, 3), "model_ms": round(model, 4),
                  "ratio": round(call["median"] / model, 4),
                  "identity_outputs": int((out == 0).all(dim=1).sum().item())})
            del g, out
        del fg0, fg, fp, fb
    eng.close()
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
