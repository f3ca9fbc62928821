"""HBM traffic per launch of the fill and eval kernels from two rocprofv3 --pmc passes
(FETCH_SIZE and WRITE_SIZE collected in separate runs, as MI355X_MICROARCH.md prescribes).

gfx950 corrections (MI355X_MICROARCH.md §HBM): FETCH_SIZE counts exactly half the bytes of a
wide (16 B/lane) coalesced streaming read, so it is doubled; WRITE_SIZE is exact for 16 B/lane
streaming stores. Both are in KiB.

    python tools/pmc_traffic.py <fetch_dir> <write_dir> <key_suffix> [out.json]
key_suffix e.g. 262144_12 -> keys fill_262144_12, eval_262144_12, fill_eval_262144_12 (what
bench.py looks up; the fused call's repeat, advice-only launch) and fill_eval_full_262144_12 (its
first, full launch).
"""
import collections
import csv
import glob
import json
import os
import sys


names_of = collections.defaultdict(set)  # kind -> the kernel names aggregated into it


def per_kernel(d, counter):
    """Per kind: the sum over its kernels of each kernel's average per dispatch (a call of the
    kind launches each of its kernels once)."""
    vals = collections.defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        per_dispatch = collections.defaultdict(float)
        names = {}
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            k = r["Kernel_Name"]
            # the fused path is two launches per step (half-round tiles, then the edge regions);
            # the eval is the fast pass (half-round + edge launches) and the gated exact kernel
            kind = ("fill" if "fill_kernel" in k
                    else "eval_part" if ("eval_hr_kernel" in k or "eval_edge_kernel" in k) else "eval" if "eval_kernel" in k
                    else "fill_eval_edge" if ("fused_kernel<27, 2>" in k or "fused_edge_kernel" in k)
                    else "fill_eval_full" if "fused_hr_kernel<27>" in k
                    else "fill_eval" if ("fused_kernel" in k or "fused_hr_kernel" in k) else None)
            if kind is None:
                continue
            per_dispatch[r["Dispatch_Id"]] += float(r["Counter_Value"])
            nm = k.replace("(anonymous namespace)::", "")
            nm = (nm[5:] if nm.startswith("void ") else nm).split("(")[0]
            names[r["Dispatch_Id"]] = (kind, nm)
            names_of[kind].add(nm)
        for disp, v in per_dispatch.items():
            vals[names[disp]].append(v)
    out = collections.defaultdict(float)
    for (kind, _), v in vals.items():
        if v:
            out[kind] += sum(v) / len(v)
    return dict(out)


def main():
    fetch_dir, write_dir, suffix = sys.argv[1:4]
    out = sys.argv[4] if len(sys.argv) > 4 else "profiles/pmc_traffic.json"
    fetch = per_kernel(fetch_dir, "FETCH_SIZE")
    write = per_kernel(write_dir, "WRITE_SIZE")
    # the fused path is two launches per step (half-round tiles, then init/final/zero tiles)
    for kk in ("fill_eval_edge", "eval_part"):
        names_of[{"fill_eval_edge": "fill_eval", "eval_part": "eval"}[kk]] |= names_of.pop(kk, set())
    # The fused call has two instantiations: the full launch (every column) on a batch's first call
    # and the advice-only one (fused_hr_kernel<59>, the fixed column left in place) on its repeat
    # calls, which is what the benchmark's timed steps run: fill_eval is the repeat call,
    # fill_eval_full the first. A library with the full launch only has one, under fill_eval.
    for d in (fetch, write):
        if "fill_eval_full" in d and "fill_eval" not in d:
            d["fill_eval"] = d.pop("fill_eval_full")
    if "fill_eval" not in names_of and "fill_eval_full" in names_of:
        names_of["fill_eval"] = names_of.pop("fill_eval_full")
    for d in (fetch, write):
        if "fill_eval_edge" in d:
            d["fill_eval"] = d.get("fill_eval", 0.0) + d.pop("fill_eval_edge")
        if "eval_part" in d:  # the fast pass (its edge walk inside the half-round launch since
            d["eval"] = d.get("eval", 0.0) + d.pop("eval_part")  # round 6) + the gated exact kernel
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zk-odst_amd"))
    from b2f import _lib

    stamp = _lib.source_stamp()
    res = json.load(open(out)) if os.path.exists(out) else {}
    for kind in ("fill", "eval", "fill_eval", "fill_eval_full"):
        if kind not in fetch or kind not in write:
            continue
        fb = 2.0 * fetch[kind] * 1024  # gfx950: FETCH_SIZE reads half of a wide stream
        wb = write[kind] * 1024
        res["%s_%s" % (kind, suffix)] = {
            "fetch_size_kib_raw": fetch[kind], "write_size_kib": write[kind],
            "fetch_bytes_corrected": fb, "write_bytes": wb, "hbm_bytes_per_launch": fb + wb,
            "correction": "FETCH_SIZE x2 (gfx950 wide-read undercount), KiB x1024",
            "kernels": sorted(names_of[kind]), "source_stamp": stamp}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
