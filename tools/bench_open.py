"""Throughput of the evaluation / opening calls (b2f_poly_eval_dev, b2f_poly_combine_dev,
b2f_kate_divide_dev) at k = 17: both fields, Montgomery form, HIP-event times (b2f_kernel_times) of
repeated calls. One JSON line per (case, field), appended to profiles/open_bench.jsonl, with the
bytes the call must move, the field products it must do, and the two floors of
tools/bench_quotient.py measured in the same process:

  copy_floor_ms     the same number of bytes as a device-to-device copy (half read, half
                    written), timed here;
  product_floor_ms  the call's field products over the rate of tools/mulbench.hip's field::mul loop
                    on this box (--mul-gps PALLAS,BN254 or the built tools/mulbench binary, run as a
                    child process before this one opens the GPU).

Cases (n = 2^k coefficients per column):
  eval_gate_queries   10 columns at the chip's own query list (b2f_gate_queries, 67 queries)
  eval_30x1           30 columns at one point each
  combine_8           8 inputs into one output
  divide_1/3/12       one column divided by 1, 3 and 12 points
`bytes` is what the call must move: every input column once, every output once (the evaluations'
outputs are a few elements: not counted). `products` is what the arithmetic needs at the least:
  eval      n per (column, point) pair (Horner)
  combine   n per term
  divide    n per point (the recurrence)
`kernel_products` is what the kernels actually do per coefficient, counted from b2f_open.hip:
  eval      1 per pair (3 Horner steps and one z^l per thread of 4 coefficients)
  divide    per point: 1 in the tile sums + 16 / 4 in the apply pass (3 for the thread's value, 6 scan
            steps, up to 3 across the waves, 1 for the carry, 3 for the recurrence)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_quotient import _stats, copy_ms, mulbench_rates  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--mul-gps", default="", help="PALLAS,BN254 G products/s of tools/mulbench")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_bench.jsonl"))
    args = ap.parse_args()
    if args.mul_gps:
        mul = tuple(float(v) for v in args.mul_gps.split(","))
        mul_src = "given"
    else:
        mul = mulbench_rates()  # a child process, before this one opens the GPU
        mul_src = "tools/mulbench, this session"
    import torch

    import b2f
    from b2f import _lib, field

    k = args.k
    n = 1 << k
    eng = b2f.Engine(0)
    s = torch.cuda.current_stream().cuda_stream
    want = set(c for c in args.cases.split(",") if c)
    lines = []

    def timed(fn):
        eng.set_timing(True)
        fn()
        eng.sync(s)
        return eng.kernel_times()["quotient"][0]

    def measure(fn):
        timed(fn)  # warm: grows the scratch
        ms = [timed(fn) for _ in range(args.reps)]
        eng.set_timing(False)
        return _stats(ms)

    def rand(cols, rows):
        return torch.randint(0, 2**60, (cols, rows, 4), dtype=torch.int64, device="cuda:0")

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        f = field.of_form(form)
        p = field.MODULUS[f]
        x = 0x123456789abcdef0123456789abcdef % p
        pts = [pow(x, i + 2, p) for i in range(30)]
        cols = rand(30, n)
        out = torch.empty((1, n, 4), dtype=torch.int64, device="cuda:0")

        def record(case, cols_in, cols_out, products, kernel_products, st):
            nbytes = 32 * n * (cols_in + cols_out)
            med = st["median"]
            rec = {"stamp": _lib.source_stamp(), "case": case, "k": k, "field": "bn254" if f else "pallas",
                   "reps": args.reps, "ms": st, "bytes": nbytes, "gbps": round(nbytes / med / 1e6, 1),
                   "copy_floor_ms": round(copy_ms(torch, nbytes), 4), "products": products,
                   "kernel_products": kernel_products}
            rec["fraction_of_copy_floor"] = round(rec["copy_floor_ms"] / med, 4)
            if mul:
                rate = mul[1 if f else 0]
                pf = products / rate / 1e6
                rec.update({"own_product_microbench_G_per_s": rate, "product_rate_source": mul_src,
                            "product_floor_ms": round(pf, 4),
                            "binding_floor": "product" if pf > rec["copy_floor_ms"] else "copy",
                            "fraction_of_binding_floor": round(max(pf, rec["copy_floor_ms"]) / med, 4)})
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)

        def on(case):
            return not want or case in want

        if on("eval_gate_queries"):
            gq = [tuple(int(v) for v in row) for row in b2f.gate_queries()]
            rot = field.rotated_points(f, x, k, range(12))
            st = measure(lambda: eng.poly_eval(cols[:10], rot, gq, form=form))
            record("eval_gate_queries", 10, 0, n * len(gq), n * len(gq), st)
        if on("eval_30x1"):
            qs = [(c, c) for c in range(30)]
            st = measure(lambda: eng.poly_eval(cols, pts, qs, form=form))
            record("eval_30x1", 30, 0, 30 * n, 30 * n, st)
        if on("combine_8"):
            terms = [[(c, pts[c]) for c in range(8)]]
            st = measure(lambda: eng.poly_combine(cols[:8], terms, form=form, out=out))
            record("combine_8", 8, 1, 8 * n, 8 * n, st)
        for m in (1, 3, 12):
            if on("divide_%d" % m):
                st = measure(lambda: eng.kate_divide(cols[:1], [pts[:m]], form=form, out=out))
                record("divide_%d" % m, 1, 1, m * n, 5 * m * n, st)
        del cols, out
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
