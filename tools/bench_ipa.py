"""Times of the IPA opening rounds (b2f_ipa_round_dev, b2f_ipa_fold_dev): both curves,
Montgomery-form scalars, HIP-event times (b2f_kernel_times) of each call, medians over --reps whole
openings. JSON lines appended to profiles/ipa_bench.jsonl, each with the source stamp and `run`
(the label given with --run), so a figure quoted elsewhere names the run it came from.

  kind = "opening"   a whole opening at 2^k: per round the round and fold medians, their sums, and a
                     host clock around the whole loop ending in one synchronise (launch gaps
                     included). Challenges are fixed on the host; there is no transcript.
                     Control, same process, interleaved per round: the round's two cross terms as two
                     single-column b2f_msm_dev calls (`two_msm_ms`; the round's own time also holds
                     its inner products). Floor: the field products the round and fold need and the
                     time they would take at tools/mulbench's rate (a child process run before this
                     one opens the GPU; scalar fields measured, base fields ASSUMED equal). Counting:
                     a Pippenger round is bench_msm.products_of(half, plan) x 2 columns + len / 2 x 2
                     products of the inner products; a direct round is (9 x 255 + 10 x 128 + 14) per
                     element of p; a fold is 2 products per row pair + (9 x 255 + 10 x adds + 10) per
                     collapsed point, adds = the set bits of u.
  kind = "sweep"     (--sweep 5,6,..) the diagnostics library forced all-direct and all-Pippenger
                     (B2F_DIAG_IPA_DIRECT) on one round of each length, interleaved: the crossing
                     point is ipa_direct_max_len (b2f_ipa.hip).
  kind = "ablation"  (--ablate-lib PATH, a build with -DB2F_IPA_NO_AFFINE) the fold with and without
                     the collapse's per-lane inversion, interleaved."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_msm import products_of  # noqa: E402
from bench_quotient import _stats, mulbench_rates  # noqa: E402

BASE_POINTS = 1 << 12  # distinct bases, tiled to len: the cost of a call does not depend on them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", default="", help="log2 of the round lengths to run on both paths")
    ap.add_argument("--ablate-lib", default="", help="a library built with -DB2F_IPA_NO_AFFINE")
    ap.add_argument("--mul-gps", default="", help="PALLAS,BN254 G products/s of tools/mulbench")
    ap.add_argument("--run", default="unnamed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_bench.jsonl"))
    args = ap.parse_args()
    if args.mul_gps:
        mul = tuple(float(v) for v in args.mul_gps.split(","))
        mul_src = "given (scalar fields); base fields assumed equal, not measured"
    else:
        mul = mulbench_rates()  # a child process, before this one opens the GPU
        mul_src = "tools/mulbench, this session (scalar fields); base fields assumed equal, not measured"
    import random

    import numpy as np
    import torch

    import b2f
    import msm_ref as mr
    from b2f import _lib

    ks = [int(v) for v in args.ks.split(",") if v]
    sweep = [int(v) for v in args.sweep.split(",") if v]
    eng = b2f.Engine(0)
    s = torch.cuda.current_stream().cuda_stream
    direct_max = _lib.ipa_direct_max_len()
    max_len = 1 << max(ks + sweep + [1])
    lines = []

    def emit(rec):
        rec = dict({"stamp": _lib.source_stamp(), "run": args.run, "reps": args.reps}, **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(e, fn):
        e.set_timing(True)
        fn()
        e.sync(s)
        return e.kernel_times()["quotient"][0]

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        cv = mr.curve_of_form(form)
        r = mr.ORDER[cv]
        curve = "bn254_g1" if cv else "vesta"
        rng = random.Random(5 + cv)
        _, pts = mr.known_bases(form, BASE_POINTS, incremental=True)
        base = torch.from_numpy(mr.pack_points(cv, pts).view(np.int64)).to("cuda:0")
        g0 = base.repeat(max_len // BASE_POINTS + 1, 1)[:max_len].contiguous()
        # random 253-bit values are below both moduli; used as Montgomery residues
        p0 = torch.randint(-2**63, 2**63 - 1, (max_len, 4), dtype=torch.int64, device="cuda:0")
        p0[:, 3] = (p0[:, 3] >> 3) & (2**61 - 1)
        x = rng.randrange(1, r)
        lr = torch.empty((2, 8), dtype=torch.int64, device="cuda:0")
        vals = torch.empty((2, 4), dtype=torch.int64, device="cuda:0")
        out1 = torch.empty((1, 8), dtype=torch.int64, device="cuda:0")

        for k in ks:
            n = 1 << k
            us = [rng.randrange(1, r) for _ in range(k)]
            b0 = eng.ipa_powers(x, n, form=form)
            p, b, g = p0[:n].clone(), b0.clone(), g0[:n].clone()
            rounds = [{"round": j, "len": n >> j, "round_ms": [], "fold_ms": [], "two_msm_ms": []} for j in range(k)]
            wall = []
            for rep in range(args.reps + 1):  # the first pass warms every shape and grows the scratch
                p.copy_(p0[:n]), b.copy_(b0), g.copy_(g0[:n])
                ln = n
                for j, u in enumerate(us):
                    P, B, G = p.data_ptr(), b.data_ptr(), g.data_ptr()
                    half = ln // 2
                    t_round = timed(eng, lambda: eng.ipa_round_dev(P, B, G, ln, form, lr.data_ptr(), vals.data_ptr(), s))
                    t_two = None
                    if ln > direct_max:
                        t_two = timed(eng, lambda: eng.msm_dev(P + 32 * half, half, half, 1, G, half, form,
                                                               out1.data_ptr(), s)) + \
                            timed(eng, lambda: eng.msm_dev(P, half, half, 1, G + 64 * half, half, form,
                                                           out1.data_ptr(), s))
                    t_fold = timed(eng, lambda: eng.ipa_fold_dev(P, B, G, ln, u, form, s))
                    if rep:
                        rounds[j]["round_ms"].append(t_round)
                        rounds[j]["fold_ms"].append(t_fold)
                        if t_two is not None:
                            rounds[j]["two_msm_ms"].append(t_two)
                    ln = half
                eng.set_timing(False)
                # the same loop untimed, one synchronise at the end: what a caller without a transcript waits
                p.copy_(p0[:n]), b.copy_(b0), g.copy_(g0[:n])
                eng.sync(s)
                t0 = time.perf_counter()
                ln = n
                for u in us:
                    eng.ipa_round_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), ln, form, lr.data_ptr(),
                                      vals.data_ptr(), s)
                    eng.ipa_fold_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), ln, u, form, s)
                    ln //= 2
                eng.sync(s)
                if rep:
                    wall.append((time.perf_counter() - t0) * 1e3)
            tot_round = tot_fold = tot_two = tot_round_long = prods_total = 0.0
            per_round = []
            for j, rd in enumerate(rounds):
                ln, half = rd["len"], rd["len"] // 2
                adds = bin(us[j]).count("1")
                fold_prods = 2 * half + (9 * 255 + 10 * adds + 10) * half
                if ln > direct_max:
                    plan = _lib.msm_plan(half, 2, form)
                    round_prods = products_of(half, plan) * 2 + 2 * half
                    path = "pippenger"
                else:
                    round_prods = (9 * 255 + 10 * 128 + 14) * ln + 2 * half
                    path = "direct"
                rec = {"round": j, "len": ln, "path": path, "round_ms": _stats(rd["round_ms"]),
                       "fold_ms": _stats(rd["fold_ms"]), "round_products": round_prods, "fold_products": fold_prods}
                tot_round += rec["round_ms"]["median"]
                tot_fold += rec["fold_ms"]["median"]
                prods_total += round_prods + fold_prods
                if rd["two_msm_ms"]:
                    rec["two_msm_ms"] = _stats(rd["two_msm_ms"])
                    tot_two += rec["two_msm_ms"]["median"]
                    tot_round_long += rec["round_ms"]["median"]
                if mul:
                    rec["round_floor_ms"] = round(round_prods / mul[cv] / 1e6, 4)
                    rec["fold_floor_ms"] = round(fold_prods / mul[cv] / 1e6, 4)
                per_round.append(rec)
            rec = {"kind": "opening", "curve": curve, "k": k, "direct_max_len": direct_max,
                   "rounds_ms": round(tot_round, 4), "folds_ms": round(tot_fold, 4),
                   "opening_ms": round(tot_round + tot_fold, 4), "wall_ms": _stats(wall),
                   "long_rounds_ms": round(tot_round_long, 4), "long_rounds_as_two_msm_ms": round(tot_two, 4),
                   "products": int(prods_total), "per_round": per_round}
            if mul:
                floor = prods_total / mul[cv] / 1e6
                rec.update({"own_product_microbench_G_per_s": mul[cv], "product_rate_source": mul_src,
                            "product_floor_ms": round(floor, 4),
                            "time_over_product_floor": round((tot_round + tot_fold) / floor, 3)})
            emit(rec)
            del p, b, g, b0

        if sweep:
            deng = b2f.Engine(0, diag=True)
            for lg in sweep:
                ln = 1 << lg
                b0 = eng.ipa_powers(x, ln, form=form)
                eng.sync(s)
                P, B, G = p0.data_ptr(), b0.data_ptr(), g0.data_ptr()
                ms = {"4294967296": [], "0": []}
                for rep in range(args.reps + 1):
                    for forced in ms:  # interleaved
                        os.environ["B2F_DIAG_IPA_DIRECT"] = forced
                        t = timed(deng, lambda: deng.ipa_round_dev(P, B, G, ln, form, lr.data_ptr(), vals.data_ptr(), s))
                        if rep:
                            ms[forced].append(t)
                os.environ.pop("B2F_DIAG_IPA_DIRECT", None)
                deng.set_timing(False)
                emit({"kind": "sweep", "curve": curve, "len": ln, "direct_ms": _stats(ms["4294967296"]),
                      "pippenger_ms": _stats(ms["0"])})
            deng.close()

        if args.ablate_lib:
            aeng = b2f.Engine(0, lib_path=args.ablate_lib)
            for k in ks:
                n = 1 << k
                u = rng.randrange(1, r)
                b0 = eng.ipa_powers(x, n, form=form)
                p, g = p0[:n].clone(), g0[:n].clone()
                ms = {"full": [], "no_affine": []}
                for rep in range(args.reps + 1):
                    for name, e in (("full", eng), ("no_affine", aeng)):  # interleaved
                        g.copy_(g0[:n])
                        t = timed(e, lambda: e.ipa_fold_dev(p.data_ptr(), b0.data_ptr(), g.data_ptr(), n, u, form, s))
                        if rep:
                            ms[name].append(t)
                eng.set_timing(False), aeng.set_timing(False)
                emit({"kind": "ablation", "curve": curve, "k": k, "what": "fold of len 2^k, collapse with / without to_affine",
                      "fold_ms": _stats(ms["full"]), "fold_no_affine_ms": _stats(ms["no_affine"])})
                del p, g, b0
            aeng.close()
        del g0, p0
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
