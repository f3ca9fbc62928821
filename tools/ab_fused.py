"""A/B of fused fill+eval library variants in ONE process, interleaved rep by rep (boxes and
even consecutive runs on one box differ by up to ~25 % in store rate, so variants are only
compared inside one process). Diagnostic only:
    python tools/ab_fused.py --libs zk-odst_amd/variants/libb2f_a.so,... [--modes 27,2,0]
The product library's split path (fill + eval) is timed in the same loop as the reference.
--resident times the product library twice per rep, fixed_resident=False (every call writes the
fixed column) beside the automatic mode (repeat calls leave it in place), and reports the reps
after the first (which carries the warm-up) as min / median / max:
    python tools/ab_fused.py --libs zk-odst_amd/variants/libb2f_parent.so --resident --reps 7"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="", help="comma-separated variant libraries (diag builds)")
    ap.add_argument("--modes", default="27", help="B2F_DIAG_FUSED modes to time per variant")
    ap.add_argument("--batch", type=int, default=1 << 18)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--mix", action="store_true", help="rounds uniform in {1,4,12} (config 5)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eval", action="store_true", help="also time each variant's eval kernel")
    ap.add_argument("--fill", action="store_true", help="also time each variant's split fill")
    ap.add_argument("--resident", action="store_true",
                    help="product library: fixed_resident=False beside the automatic mode")
    args = ap.parse_args()
    import torch

    import b2f
    from b2f import synth

    x = synth.batch(args.batch, rounds=args.rounds, rounds_mix=[1, 4, 12] if args.mix else None)
    batch = b2f.DeviceBatch(x)
    s = torch.cuda.current_stream().cuda_stream
    prod = b2f.Engine(0)
    engines = [("product", prod)]
    envs = {}
    for spec in [v for v in args.libs.split(",") if v]:
        # path[@K=V[;K=V]]: environment set around that variant's fused calls (diag builds)
        p, _, env = spec.partition("@")
        name = os.path.basename(p)[6:-3] + ("@" + env if env else "")
        engines.append((name, b2f.Engine(0, lib_path=os.path.join(ROOT, p))))
        envs[name] = dict(kv.split("=", 1) for kv in env.split(";") if kv)
    nbytes = batch.used_rows * 44
    batch.fill(prod, s)
    batch.evaluate(prod, s)
    prod.sync(s)
    res = {}
    paths = {}
    modes = [m for m in args.modes.split(",") if m]
    for rep in range(args.reps):
        prod.set_timing(True)
        batch.fill(prod, s)
        batch.evaluate(prod, s)
        kt = prod.kernel_times()
        res.setdefault("split(fill+eval)", []).append(kt["fill"][0] + kt["eval"][0] + kt["record"][0])
        if args.resident:
            # One batch for every configuration (a second 60 GB allocation was measured 14 %
            # slower to write with the same kernel). Every timed call follows an untimed call of
            # its own kind, so none is timed in the wake of another's kernels (straight after the
            # split eval the same kernel measured 2.9 % slower), and the order rotates from rep to
            # rep. The automatic mode's lead call runs in full wherever another engine's call or
            # the split fill came before it; its timed call then leaves the column in place.
            cfgs = [("product/fused27/full", prod, {"fixed_resident": False}),
                    ("product/fused27/auto", prod, {})]
            cfgs += [("%s/fused27" % name, eng, {}) for name, eng in engines[1:]]
            for j in range(len(cfgs)):
                key, eng, kw = cfgs[(rep + j) % len(cfgs)]
                batch.fill_evaluate(eng, s, **kw)
                eng.set_timing(True)
                batch.fill_evaluate(eng, s, **kw)
                if eng is prod:
                    paths.setdefault(key, set()).add(eng.debug_fused_path())
                kt = eng.kernel_times()
                res.setdefault(key, []).append(kt["fill_eval"][0] + kt["record"][0])
                eng.sync(s)
            continue
        for name, eng in engines:
            for k, v in envs.get(name, {}).items():
                os.environ[k] = v
            if args.fill:
                eng.set_timing(True)
                batch.fill(eng, s)
                kt = eng.kernel_times()
                res.setdefault("%s/fill" % name, []).append(kt["fill"][0])
                eng.sync(s)
            if args.eval:
                eng.set_timing(True)
                batch.evaluate(eng, s)
                kt = eng.kernel_times()
                res.setdefault("%s/eval" % name, []).append(kt["eval"][0])
                eng.sync(s)
            for m in modes if name != "product" else ["27"]:
                os.environ["B2F_DIAG_FUSED"] = m
                eng.set_timing(True)
                batch.fill_evaluate(eng, s)
                kt = eng.kernel_times()
                res.setdefault("%s/fused%s" % (name, m), []).append(kt["fill_eval"][0] + kt["record"][0])
                eng.sync(s)
            for k in envs.get(name, {}):
                os.environ.pop(k, None)
        os.environ.pop("B2F_DIAG_FUSED", None)
    for k, v in res.items():
        best = min(v)
        print("%-28s min %8.3f ms  (%6.0f GB/s)  all %s" % (k, best, nbytes / best / 1e6,
                                                         ["%.2f" % t for t in v]))
    if args.resident:
        import statistics

        print("reps after the first: min / median / max ms")
        for k, v in res.items():
            if len(v) > 1:
                print("%-28s %8.3f %8.3f %8.3f" % (k, min(v[1:]), statistics.median(v[1:]), max(v[1:])))
        print("fused paths of the timed calls (0 full, 1 advice-only):", paths)
    rep = batch.report_dict()
    print("last verdict clean:", rep["first_failure"] == 2**64 - 1)


if __name__ == "__main__":
    main()
