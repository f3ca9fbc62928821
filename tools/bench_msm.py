"""Throughput of the commitments (b2f_msm_dev): both curves, Montgomery-form scalars, HIP-event
times (b2f_kernel_times) of repeated calls. One JSON line per (curve, len, n_cols, distribution),
appended to profiles/msm_bench.jsonl, with the plan, the field products the plan needs and the
time those would take at the product rate of tools/mulbench.hip's field::mul loop on this box
(--mul-gps PALLAS,BN254 or the built tools/mulbench binary, run as a child process before this one
opens the GPU). mulbench measures the SCALAR fields' products; the base fields' rate is ASSUMED
equal (VestaBase has pallas' generated shortcuts, Bn254Base is a full product like BN254's) and
not measured: `product_rate_source` says so in every line.

Distributions (n_cols columns of len scalars):
  uniform   random elements of the scalar field
  ones      every scalar 1 (a selector-like column: one bucket of window 0 holds every row)
  advice    a real advice column of the chip (the dense 16-bit limbs of a filled batch, exported
            with b2f_export_fp_dev), rotated by a few rows per column
`products` per column, for digits = len x windows entries (uniform scalars leave 2^-c of them
zero; not discounted):
  bucket level 0   10 per digit (one mixed addition)
  levels above     14 x 2 digits / 32 x (1 + 1/16 + ..) = 14 digits / 15 (full additions)
  windows          14 x 2 per bucket (running sums) x windows x 2^(c-1)
  Horner           9 x 256 doublings + 14 per window
--sweep: the forced plan (diagnostics library, B2F_DIAG_MSM_PLAN) over window widths at n_cols = 8,
uniform scalars: the line of each width, from which msm_default_window (b2f_msm.hip) is chosen."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_quotient import _stats, mulbench_rates  # noqa: E402

BASE_POINTS = 1 << 15  # distinct bases, tiled to len: the cost of a call does not depend on them


def products_of(ln, plan):
    c, w = plan["window_bits"], plan["windows"]
    digits = ln * w
    return int(10 * digits + 14 * digits / 15 + 28 * w * (1 << (c - 1)) + 9 * 256 + 14 * w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", default="17,20", help="log2 of the lengths")
    ap.add_argument("--cols", default="1,8,32")
    ap.add_argument("--dists", default="uniform,ones,advice")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", default="", help="window widths to force, e.g. 9,10,11,12,13,14,15,16")
    ap.add_argument("--mul-gps", default="", help="PALLAS,BN254 G products/s of tools/mulbench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_bench.jsonl"))
    args = ap.parse_args()
    if args.mul_gps:
        mul = tuple(float(v) for v in args.mul_gps.split(","))
        mul_src = "given (scalar fields); base fields assumed equal, not measured"
    else:
        mul = mulbench_rates()  # a child process, before this one opens the GPU
        mul_src = "tools/mulbench, this session (scalar fields); base fields assumed equal, not measured"
    import numpy as np
    import torch

    import b2f
    import msm_ref as mr
    from b2f import _lib, synth

    sweep = [int(v) for v in args.sweep.split(",") if v]
    eng = b2f.Engine(0, diag=bool(sweep))
    s = torch.cuda.current_stream().cuda_stream
    lens = [1 << int(v) for v in args.lens.split(",")]
    cols_list = [8] if sweep else [int(v) for v in args.cols.split(",")]
    dists = ["uniform"] if sweep else args.dists.split(",")
    max_len, max_cols = max(lens), max(cols_list)
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

    for form in (_lib.FP_MONTGOMERY, _lib.FP_BN254_MONTGOMERY):
        cv = mr.curve_of_form(form)
        r = mr.ORDER[cv]
        _, pts = mr.known_bases(form, BASE_POINTS, incremental=True)
        base = torch.from_numpy(mr.pack_points(cv, pts).view(np.int64)).to("cuda:0")
        bases = base.repeat(max_len // BASE_POINTS + 1, 1)[:max_len].contiguous()
        data = {}
        if "uniform" in dists:  # random 253-bit values are below both moduli; used as Montgomery residues
            u = torch.randint(-2**63, 2**63 - 1, (max_cols, max_len, 4), dtype=torch.int64, device="cuda:0")
            u[:, :, 3] = (u[:, :, 3] >> 3) & (2**61 - 1)
            data["uniform"] = u
        if "ones" in dists:
            one = torch.from_numpy(mr.pack_scalars(form, [1]).view(np.int64)).to("cuda:0")
            data["ones"] = one.reshape(1, 1, 4).repeat(max_cols, max_len, 1).contiguous()
        if "advice" in dists:
            x = synth.batch(max_len // 5220 + 2, rounds_mix=[12])
            batch = b2f.DeviceBatch(x, device="cuda:0")
            batch.fill(eng)
            col = batch.export_fp(eng, 0, max_len, form=form)[b2f.halo2_column_index(1)]  # a_1: dense limbs
            data["advice"] = torch.stack([torch.roll(col, 3 * i, 0) for i in range(max_cols)]).contiguous()
            del batch
        for ln in lens:
            for n_cols in cols_list:
                for dist in dists:
                    for c in (sweep or [0]):
                        if c:
                            os.environ["B2F_DIAG_MSM_PLAN"] = str(c)
                        try:
                            plan = _lib.msm_plan(ln, n_cols, form, diag=bool(sweep))
                            sc = data[dist][:n_cols]
                            out = torch.empty((n_cols, 8), dtype=torch.int64, device="cuda:0")
                            st = measure(lambda: eng.msm_dev(sc.data_ptr(), max_len, ln, n_cols, bases.data_ptr(),
                                                             ln, form, out.data_ptr(), s))
                        finally:
                            os.environ.pop("B2F_DIAG_MSM_PLAN", None)
                        med = st["median"]
                        prods = products_of(ln, plan) * n_cols
                        rec = {"stamp": _lib.source_stamp(), "curve": "bn254_g1" if cv else "vesta", "len": ln,
                               "n_cols": n_cols, "dist": dist, "forced_c": c, "plan": plan, "reps": args.reps,
                               "ms": st, "ms_per_column": round(med / n_cols, 4),
                               "Mscalars_per_s": round(ln * n_cols / med / 1e3, 2), "products": prods}
                        if mul:
                            rate = mul[cv]
                            rec.update({"own_product_microbench_G_per_s": rate, "product_rate_source": mul_src,
                                        "product_floor_ms": round(prods / rate / 1e6, 4),
                                        "fraction_of_product_floor": round(prods / rate / 1e6 / med, 4)})
                        lines.append(json.dumps(rec))
                        print(lines[-1], flush=True)
        del data, bases
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
