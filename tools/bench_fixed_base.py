"""Times of the fixed-base multiples (b2f_fixed_base_mul_dev) and of the KZG set-up built on them
(Engine.kzg_setup): both curves, HIP-event times (b2f_kernel_times) of whole calls, medians over
--reps calls after a warm-up. JSON lines appended to profiles/fixed_base_bench.jsonl, each with the
source stamp and `run` (the label given with --run).

  kind = "fixed_base"  one case (curve, len): first_ms, the first call with a fresh base (the
                       table build and the multiples in one region); call_ms, the steady state (same
                       base, table cached); t_sm, measured in the same process and interleaved with
                       the calls: b2f_ipa_fold_dev at len = 2^21 collapses 2^20 points, each one
                       general scalar multiplication, so t_sm = t_fold / 2^20;
                       ratio = (call / len) / t_sm, expected <= 0.25 at len = 2^20. one_digit_ms is
                       the same call on scalars of one non-zero digit (one table entry, no addition,
                       one affine conversion): what the per-lane inversion and the launch cost
                       without the additions. identity_outputs counts all-zero points.
  kind = "table"       the table build alone, as first_ms - call_ms at the smallest len.
  kind = "kzg_setup"   (curve, k): the three calls of Engine.kzg_setup, one region each: the powers
                       of tau, the multiples (table cached: built by the cases above), the group
                       NTT."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", default="12,16,20", help="log2 of the lengths")
    ap.add_argument("--setup-ks", default="17,20")
    ap.add_argument("--curves", default="vesta,bn254_g1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="unnamed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_base_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    import random

    import numpy as np
    import torch

    import b2f
    import msm_ref as mr
    from b2f import _lib, curve, field

    logs = [int(v) for v in args.lens.split(",") if v]
    setup_ks = [int(v) for v in args.setup_ks.split(",") if v]
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

    def scalars(n, seed):
        g = torch.Generator(device="cuda:0").manual_seed(seed)
        v = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device="cuda:0", generator=g)
        v[:, 3] = (v[:, 3] >> 3) & (2**61 - 1)  # 253-bit values are below both moduli
        return v

    for form in (_lib.FP_CANONICAL, _lib.FP_BN254_CANONICAL):  # canonical: the digits are the limbs' bytes
        cv = mr.curve_of_form(form)
        name = "bn254_g1" if cv else "vesta"
        if name not in args.curves.split(","):
            continue
        r = mr.ORDER[cv]
        rng = random.Random(19 + cv)
        plan = _lib.fixed_base_plan(1, form)
        # the yardstick: one fold of 2^21, i.e. 2^20 general scalar multiplications
        _, pts = mr.known_bases(form, BASE_POINTS, incremental=True)
        base = torch.from_numpy(mr.pack_points(cv, pts).view(np.int64)).to("cuda:0")
        fn_ = 1 << FOLD_LOG
        i = torch.arange(fn_, dtype=torch.int64, device="cuda:0")
        fg0 = base[(i + 17 * (i >> 12) + 5 * (i >> 12) * (i >> 12)) % BASE_POINTS].contiguous()
        fg, fp = fg0.clone(), scalars(fn_, 5)
        fb = fp.clone()
        us = [rng.randrange(1, r) for _ in range(args.reps + 1)]

        def fold(rep):
            fg.copy_(fg0)
            return timed(lambda: eng.ipa_fold_dev(fp.data_ptr(), fb.data_ptr(), fg.data_ptr(), fn_, us[rep], form, s))

        gen = curve.pack_points(cv, [curve.GENERATOR[cv]])[0]
        table_ms = None
        for lg in logs:
            n = 1 << lg
            sc = scalars(n, 100 + lg)
            one = torch.zeros_like(sc)
            one[:, (lg % 4)] = 1 << 40  # one non-zero digit
            out = torch.empty((n, 8), dtype=torch.int64, device="cuda:0")
            fresh = mr.pack_points(cv, [mr.gen_mul(cv, rng.randrange(2, r))])[0]
            first = timed(lambda: eng.fixed_base_mul_dev(fresh, sc.data_ptr(), n, form, out.data_ptr(), s))
            t_call, t_one, t_fold = [], [], []
            for rep in range(args.reps + 1):  # the first pass warms
                tf = fold(rep)
                tc = timed(lambda: eng.fixed_base_mul_dev(gen, sc.data_ptr(), n, form, out.data_ptr(), s))
                to = timed(lambda: eng.fixed_base_mul_dev(gen, one.data_ptr(), n, form, out.data_ptr(), s))
                if rep:
                    t_fold.append(tf)
                    t_call.append(tc)
                    t_one.append(to)
            eng.fixed_base_mul_dev(gen, sc.data_ptr(), n, form, out.data_ptr(), s)
            eng.sync(s)
            call, onem, foldm = _stats(t_call), _stats(t_one), _stats(t_fold)
            t_sm = foldm["median"] / (fn_ // 2)
            steady_fresh = timed(lambda: eng.fixed_base_mul_dev(fresh, sc.data_ptr(), n, form, out.data_ptr(), s))
            if table_ms is None:
                table_ms = round(first - steady_fresh, 4)
            emit({"kind": "fixed_base", "curve": name, "len_log2": lg, "window_bits": plan["window_bits"],
                  "table_bytes": plan["scratch_bytes"], "first_ms": round(first, 4), "call_ms": call,
                  "per_output_ns": round(call["median"] / n * 1e6, 3), "one_digit_ms": onem, "fold_len": fn_,
                  "fold_ms": foldm, "t_sm_ns": round(t_sm * 1e6, 3), "ratio": round(call["median"] / n / t_sm, 4),
                  "identity_outputs": int((out == 0).all(dim=1).sum().item())})
            del sc, one, out
        emit({"kind": "table", "curve": name, "build_ms": table_ms, "points": plan["table_points"]})
        del fg0, fg, fp, fb
        mform = form | 1
        for k in setup_ks:
            n = 1 << k
            tau = rng.randrange(2, r)
            omega = field.omega(field.of_form(mform), k)
            pw = torch.empty((n, 4), dtype=torch.int64, device="cuda:0")
            g = torch.empty((n, 8), dtype=torch.int64, device="cuda:0")
            lag = torch.empty_like(g)
            parts = [[], [], []]
            for rep in range(args.reps + 1):
                t = [timed(lambda: eng.ipa_powers_dev(tau, n, mform, pw.data_ptr(), s)),
                     timed(lambda: eng.fixed_base_mul_dev(gen, pw.data_ptr(), n, mform, g.data_ptr(), s)),
                     timed(lambda: eng.group_ntt_dev(g.data_ptr(), k, omega, _lib.NTT_INVERSE, mform, lag.data_ptr(), s))]
                if rep:
                    for p_, v in zip(parts, t):
                        p_.append(v)
            st = [_stats(p_) for p_ in parts]
            emit({"kind": "kzg_setup", "curve": name, "k": k, "powers_ms": st[0], "fixed_base_ms": st[1],
                  "group_ntt_ms": st[2], "total_ms": round(sum(x["median"] for x in st), 4)})
            del pw, g, lag
    eng.set_timing(False)
    eng.close()
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
