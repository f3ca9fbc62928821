"""Throughput of the batched NTT (b2f_ntt_columns_dev): forward (onto a coset) and inverse, both
fields, Montgomery form, HIP-event times (b2f_kernel_times) of repeated calls with warm tables.
One JSON line per (shape, field, direction) with two bounds measured on the same box in the same
session:

  hbm_bound_ms      passes x 64 B x n x columns over the box's stream rate (--hbm-gbps, e.g. a
                    floor of `bench.py --full`; default: a 1 GiB device-to-device copy timed here,
                    read + write bytes);
  product_bound_ms  columns x (n/2 k + n) field products (the butterflies plus one scale per
                    element) over the rate of tools/mulbench.hip's field::mul loop on this box
                    ("own product microbench"; --mul-gps PALLAS,BN254 or the built tools/mulbench
                    binary, run as a child process before this one opens the GPU).
`executed_products` counts what the kernels run: the butterflies, two per element for every
inter-pass twiddle (table combine + multiply) and two per element for the coset / inverse scale.

The k = 17 x 64 shape is also run as 64 single-column calls in the same process, rep by rep in
turn with the batch call (`loop_ms`)."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def passes(k):
    return 1 if k <= 10 else (k + 7) // 8


def mulbench_rates():
    """(pallas, bn254) G products/s of field::mul (variant 0, best of 1 and 2 chains), or None."""
    exe = os.path.join(ROOT, "tools", "mulbench")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    best = {}
    for m in re.finditer(r"^(\w+)\s+variant 0 chains \d+: [\d.]+ ms, ([\d.]+) G products/s$", out, re.M):
        best[m.group(1)] = max(best.get(m.group(1), 0.0), float(m.group(2)))
    if "Pallas" not in best or "Bn254" not in best:
        return None
    return best["Pallas"], best["Bn254"]


def copy_rate_gbps(torch, reps=5):
    a = torch.empty(1 << 27, dtype=torch.int64, device="cuda:0")
    b = torch.empty_like(a)
    b.copy_(a)
    best = 0.0
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        best = max(best, 2 * a.numel() * 8 / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="17x64,22x1,22x8", help="k x columns, comma separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", default=None, help="a variant library (A/B), default the product")
    ap.add_argument("--hbm-gbps", type=float, default=0.0)
    ap.add_argument("--mul-gps", default="", help="PALLAS,BN254 G products/s of tools/mulbench")
    ap.add_argument("--loop-k", type=int, default=17, help="the shape also run as single-column calls")
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

    eng = b2f.Engine(0) if not args.lib else b2f.Engine(0, lib_path=args.lib)
    s = torch.cuda.current_stream().cuda_stream
    hbm = args.hbm_gbps or copy_rate_gbps(torch)
    hbm_src = "given" if args.hbm_gbps else "1 GiB device copy, this session"

    def timed(fn):
        eng.set_timing(True)
        fn()
        eng.sync(s)
        return eng.kernel_times()["ntt"][0]

    for shape in args.shapes.split(","):
        k, cols = (int(v) for v in shape.split("x"))
        n = 1 << k
        for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
            f = field.of_form(form)
            p = field.MODULUS[f]
            zeta = pow(field.GENERATOR[f], (p - 1) // 3, p)  # a cube root of unity as the coset
            x = torch.randint(0, 2**60, (cols, n, 4), dtype=torch.int64, device="cuda:0")
            y = torch.empty_like(x)
            for inverse in (False, True):
                def batch():
                    eng.ntt_columns(x, k, inverse=inverse, shift=zeta, form=form, out=y)

                def loop():
                    for c in range(cols):
                        eng.ntt_columns(x[c:c + 1], k, inverse=inverse, shift=zeta, form=form, out=y[c:c + 1])

                do_loop = k == args.loop_k and cols > 1
                timed(batch)  # builds the tables
                ms, loop_ms = [], []
                for _ in range(args.reps):
                    ms.append(timed(batch))
                    if do_loop:
                        loop_ms.append(timed(loop))
                eng.set_timing(False)
                med = _stats(ms)["median"]
                P = passes(k)
                elems = cols * n
                products = cols * (n // 2 * k + n)
                executed = cols * (n // 2 * k + 2 * n * (P - 1) + 2 * n)
                rec = {"stamp": _lib.source_stamp(), "lib": args.lib or "product", "k": k,
                       "columns": cols, "field": "bn254" if f else "pallas",
                       "direction": "inverse" if inverse else "forward", "passes": P,
                       "reps": args.reps, "ms": _stats(ms),
                       "elements_per_s": round(elems / med * 1e3),
                       "hbm_gbps": round(hbm, 1), "hbm_rate_source": hbm_src,
                       "hbm_bound_ms": round(P * 64 * elems / hbm / 1e6, 4),
                       "executed_products": executed,
                       "executed_G_products_per_s": round(executed / med / 1e6, 2)}
                if mul:
                    rate = mul[1 if f else 0]
                    pb = products / rate / 1e6
                    rec.update({"own_product_microbench_G_per_s": rate, "product_rate_source": mul_src,
                                "product_bound_ms": round(pb, 4),
                                "dominant_bound": "product" if pb > rec["hbm_bound_ms"] else "hbm",
                                "fraction_of_dominant_bound": round(max(pb, rec["hbm_bound_ms"]) / med, 4)})
                if do_loop:
                    rec["loop_ms"] = _stats(loop_ms)
                    rec["batch_over_loop"] = round(med / _stats(loop_ms)["median"], 4)
                print(json.dumps(rec), flush=True)
            del x, y
    eng.close()


if __name__ == "__main__":
    main()
