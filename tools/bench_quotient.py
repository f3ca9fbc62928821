"""Throughput of the quotient calls (b2f_quotient_gates_dev, b2f_quotient_permutation_dev,
b2f_quotient_lookup_dev, b2f_quotient_divide_dev) at k = 17, ext_k = 19: both fields, Montgomery form, chunk_len 2 and 3,
HIP-event times (b2f_kernel_times) of repeated calls with a warm X_i table. One JSON line per
(call, field, chunk_len) with the bytes the call must move, the resulting GB/s and two floors
measured in the same process:

  copy_floor_ms     the same number of bytes as a device-to-device copy (half read, half
                    written), timed here;
  product_floor_ms  rows x the call's field products per row over the rate of tools/mulbench.hip's
                    field::mul loop on this box (--mul-gps PALLAS,BN254 or the built tools/mulbench
                    binary, run as a child process before this one opens the GPU).

`bytes` counts every column element the call reads once (the rotated z and A' reads are other rows
of columns already counted: not counted again), h_in and h_out. Products per row, Montgomery form:
  permutation  4 per column (32) + per set: the l_active product, a fold, and from the second set on
               the link product and its fold + 3 for e_0, e_1 + 2 folds + X_i + the final y^sets
  lookup       12 in the terms + 5 folds
  gates        118, counted from quot_gates_kernel: 28 by the weights 2^8, 2^16, 2^30, 2^64 and
               65535, 11 in the carry and boolean polynomials, 50 Horner steps in y inside the
               gates, 16 selector products q_g y^S_g, 12 products of a gate's polynomial sum by
               its selector(s), 1 for y^74 h_in
  divide       1
For scale, `ntt_ms` is the coeff_to_extended NTT (b2f_ntt_columns_dev, k = 19, in_len = 2^17) of
the same columns the call reads, from the same run."""
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


def copy_ms(torch, nbytes, reps=7):
    """A device copy moving nbytes in all (nbytes / 2 read, nbytes / 2 written): median ms."""
    a = torch.empty(nbytes // 16, dtype=torch.int64, device="cuda:0")
    b = torch.empty_like(a)
    b.copy_(a)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


def permutation_products(chunk_len):
    sets = -(-8 // chunk_len)
    return 32 + 2 * sets + 2 * (sets - 1) + 3 + 2 + 1 + 1


GATES_PRODUCTS = 28 + 11 + 50 + 16 + 12 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=17)
    ap.add_argument("--ext-k", type=int, default=19)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--mul-gps", default="", help="PALLAS,BN254 G products/s of tools/mulbench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quotient_bench.jsonl"))
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

    k, ext_k = args.k, args.ext_k
    n, n_ext = 1 << k, 1 << ext_k
    usable = n - 6
    eng = b2f.Engine(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = []

    def timed(fn, kind):
        eng.set_timing(True)
        fn()
        eng.sync(s)
        return eng.kernel_times()[kind][0]

    def measure(fn, kind="quotient"):
        timed(fn, kind)  # warm: builds the tables
        ms = [timed(fn, kind) for _ in range(args.reps)]
        eng.set_timing(False)
        return _stats(ms)

    def rand(cols, rows):
        return torch.randint(0, 2**60, (cols, rows, 4), dtype=torch.int64, device="cuda:0")

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        f = field.of_form(form)
        p = field.MODULUS[f]
        zeta = pow(field.GENERATOR[f], (p - 1) // 3, p)  # a cube root of unity as the coset
        beta, gamma, y = 0x1234567 % p, 0x89abcdef % p, 0xfedcba987 % p
        l, adv, sigma, lk = rand(3, n_ext), rand(10, n_ext), rand(8, n_ext), rand(5, n_ext)
        h = rand(1, n_ext)[0]
        coeff = rand(10, n)  # what coeff_to_extended reads

        def ntt_ms(cols):
            out = torch.empty((cols, n_ext, 4), dtype=torch.int64, device="cuda:0")
            st = measure(lambda: eng.ntt_columns(coeff[:cols], ext_k, shift=zeta, in_len=n, form=form, out=out),
                         "ntt")
            return st["median"]

        ntt_per_col = {c: ntt_ms(c) for c in (1, 5, 8, 10)}

        def record(call, chunk_len, cols_read, products, st):
            nbytes = 32 * n_ext * (cols_read + 2)  # + h_in and h_out
            med = st["median"]
            rec = {"stamp": _lib.source_stamp(), "call": call, "k": k, "ext_k": ext_k,
                   "field": "bn254" if f else "pallas", "chunk_len": chunk_len, "reps": args.reps,
                   "ms": st, "columns_read": cols_read, "bytes": nbytes,
                   "gbps": round(nbytes / med / 1e6, 1),
                   "copy_floor_ms": round(copy_ms(torch, nbytes), 4),
                   "products_per_row": products}
            rec["fraction_of_copy_floor"] = round(rec["copy_floor_ms"] / med, 4)
            if mul:
                rate = mul[1 if f else 0]
                pf = products * n_ext / rate / 1e6
                rec.update({"own_product_microbench_G_per_s": rate, "product_rate_source": mul_src,
                            "product_floor_ms": round(pf, 4),
                            "binding_floor": "product" if pf > rec["copy_floor_ms"] else "copy",
                            "fraction_of_binding_floor": round(max(pf, rec["copy_floor_ms"]) / med, 4)})
            # the NTT that brings the same columns to the coset (8 or 10 at a time, summed)
            left, t = cols_read, 0.0
            for c in (10, 8, 5, 1):
                while left >= c:
                    t += ntt_per_col[c]
                    left -= c
            rec["ntt_ms_same_columns"] = round(t, 4)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)

        for chunk_len in (2, 3):
            sets = -(-8 // chunk_len)
            z = rand(sets, n_ext)
            st = measure(lambda: eng.quotient_permutation(k, ext_k, usable, l, adv, sigma, z, chunk_len, zeta,
                                                          beta, gamma, y, h=h, form=form))
            # the two advice columns outside the permutation are not read
            record("permutation", chunk_len, 3 + 8 + 8 + sets, permutation_products(chunk_len), st)
            del z
        st = measure(lambda: eng.quotient_lookup(k, ext_k, l, lk, beta, gamma, y, h=h, form=form))
        record("lookup", 0, 3 + 5, 17, st)
        fx = rand(_lib.NUM_FIXED_FP, n_ext)
        st = measure(lambda: eng.quotient_gates(k, ext_k, adv, fx, y, h=h, form=form))
        record("gates", 0, 10 + _lib.NUM_FIXED_FP, GATES_PRODUCTS, st)
        del fx
        st = measure(lambda: eng.quotient_divide(k, ext_k, zeta, h, form=form))
        record("divide", 0, 0, 1, st)
        del l, adv, sigma, lk, h, coeff
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
