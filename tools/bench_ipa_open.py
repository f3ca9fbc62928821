"""Wall time of a whole IPA opening as one queued call (b2f_ipa_open_dev) against the three-call
loop it replaces, both curves, Montgomery-form scalars. JSON lines appended to
profiles/ipa_open_bench.jsonl, each with the source stamp and `run` (the label given with --run).

  one_call_ms     host clock around b2f_ipa_open_dev ending in one synchronise: every round, the
                  blinded L_j / R_j, the challenges from the device transcript, c and f
  three_call_ms   host clock around k x (b2f_ipa_round_dev, b2f_ipa_fold_dev) ending in one
                  synchronise, with every challenge known in advance and NO host work between the
                  calls: no download, no U / W terms, no hash. This is the lower bound of any
                  host-driven loop, not a loop a caller could run. It is given the u_j the one call
                  squeezed, so the generator collapses do the same additions in both.

Same process, interleaved, medians over --reps after one warming pass. The per-round cost of the
blinding-and-squeeze step comes from a kernel trace of this tool (fb_blind_kernel,
ipa_challenge_kernel), not from here."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_quotient import _stats  # noqa: E402

BASE_POINTS = 1 << 12  # distinct bases, tiled to len: the cost of a call does not depend on them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run", default="unnamed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipa_open_bench.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import b2f
    import msm_ref as mr
    from b2f import _lib

    ks = [int(v) for v in args.ks.split(",") if v]
    eng = b2f.Engine(0)
    s = torch.cuda.current_stream().cuda_stream
    max_len = 1 << max(ks)
    lines = []

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda:0")

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        cv = mr.curve_of_form(form)
        r = mr.ORDER[cv]
        rng = random.Random(15 + cv)
        _, pts = mr.known_bases(form, BASE_POINTS, incremental=True)
        g0 = dev(mr.pack_points(cv, pts)).repeat(max_len // BASE_POINTS + 1, 1)[:max_len].contiguous()
        # random 253-bit values are below both moduli; used as Montgomery residues
        p0 = torch.randint(-2**63, 2**63 - 1, (max_len, 4), dtype=torch.int64, device="cuda:0")
        p0[:, 3] = (p0[:, 3] >> 3) & (2**61 - 1)
        x = rng.randrange(1, r)
        U, W = mr.pack_points(cv, [mr.gen_mul(cv, rng.randrange(1, r)), mr.gen_mul(cv, rng.randrange(1, r))])
        lr1 = torch.empty((2, 8), dtype=torch.int64, device="cuda:0")
        vals = torch.empty((2, 4), dtype=torch.int64, device="cuda:0")
        for k in ks:
            n = 1 << k
            b0 = eng.ipa_powers(x, n, form=form)
            p, b, g = p0[:n].clone(), b0.clone(), g0[:n].clone()
            rand = dev(mr.pack_scalars(form, [rng.randrange(r) for _ in range(2 * k)]))
            f0 = dev(mr.pack_scalars(form, [rng.randrange(r)]))[0]
            state0 = eng.transcript_init()
            eng.transcript_absorb_scalars(state0, rand[:3], form=form)  # any earlier content
            z = eng.transcript_squeeze(state0, form=form)
            state = state0.clone()
            lr = torch.empty((k, 16), dtype=torch.int64, device="cuda:0")
            u = torch.empty((k, 4), dtype=torch.int64, device="cuda:0")
            cf = torch.empty((2, 4), dtype=torch.int64, device="cuda:0")
            one, three, us = [], [], None
            for rep in range(args.reps + 1):  # the first pass warms every shape and grows the scratch
                p.copy_(p0[:n]), b.copy_(b0), g.copy_(g0[:n]), state.copy_(state0), cf[1].copy_(f0)
                eng.sync(s)
                t0 = time.perf_counter()
                eng.ipa_open_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), n, U, W, z.data_ptr(), rand.data_ptr(),
                                 state.data_ptr(), form, lr.data_ptr(), u.data_ptr(), cf.data_ptr(), s)
                eng.sync(s)
                if rep:
                    one.append((time.perf_counter() - t0) * 1e3)
                if us is None:
                    us = [int.from_bytes(row.tobytes(), "little") for row in u.cpu().numpy().view(np.uint64)]
                c_one = cf[0].cpu().numpy().copy()
                p.copy_(p0[:n]), b.copy_(b0), g.copy_(g0[:n])
                eng.sync(s)
                t0 = time.perf_counter()
                ln = n
                for uj in us:
                    eng.ipa_round_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), ln, form, lr1.data_ptr(),
                                      vals.data_ptr(), s)
                    eng.ipa_fold_dev(p.data_ptr(), b.data_ptr(), g.data_ptr(), ln, uj, form, s)
                    ln //= 2
                eng.sync(s)
                if rep:
                    three.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(p[0].cpu().numpy(), c_one), "the two loops disagree on c"
            rec = {"stamp": _lib.source_stamp(), "run": args.run, "reps": args.reps, "kind": "open",
                   "curve": "bn254_g1" if cv else "vesta", "k": k, "one_call_ms": _stats(one),
                   "three_call_ms": _stats(three),
                   "one_call_over_three_call": round(_stats(one)["median"] / _stats(three)["median"], 4)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del p, b, g, b0
        del g0, p0
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
