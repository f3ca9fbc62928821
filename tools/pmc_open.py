"""Summarise the counters-only rocprofv3 pass of tools/pmc_open.sh: per kernel of b2f_open.hip and
field the mean of every counter over the kernel's dispatches, one JSON line per kernel, with the
bytes the bench's case makes the kernel read once (k = 17: the evaluation kernel 10 columns, the
combine kernel 8) and FETCH_SIZE as a fraction of them. The combine kernel reads each input exactly
once by construction, so its fraction calibrates the counter; `fetch_vs_combine` is the evaluation
kernel's fraction over the combine kernel's of the same field: 1.0 means every column was fetched
once, whatever the number of queries on it.
Usage: python3 tools/pmc_open.py <dir holding the pass directory> [k]"""
import collections
import csv
import glob
import json
import re
import sys

READS = {"poly_eval_partial_kernel": 10, "poly_combine_kernel": 8}  # columns read once per dispatch


def main():
    root = sys.argv[1]
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 17
    agg = collections.OrderedDict()
    for f in sorted(glob.glob(root + "/**/*counter_collection.csv", recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"(\w+_kernel)<b2f::field::(\w+)>", r["Kernel_Name"])
                if not m or m.group(1) not in READS:
                    continue
                d = agg.setdefault((m.group(1), m.group(2).lower()), collections.defaultdict(list))
                d[r["Counter_Name"]].append(float(r["Counter_Value"]))
    recs = {}
    for (name, field), d in agg.items():
        rec = {"kernel": name, "field": field, "k": k}
        rec.update({c: round(sum(v) / len(v), 1) for c, v in sorted(d.items())})
        rec["dispatches"] = max(len(v) for v in d.values())
        rec["column_kib_read_once"] = READS[name] * (32 << k) // 1024
        if "FETCH_SIZE" in rec:
            rec["fetch_fraction"] = round(rec["FETCH_SIZE"] / rec["column_kib_read_once"], 4)
        recs[(name, field)] = rec
    for (name, field), rec in recs.items():
        cal = recs.get(("poly_combine_kernel", field), {}).get("fetch_fraction")
        if name == "poly_eval_partial_kernel" and cal and "fetch_fraction" in rec:
            rec["fetch_vs_combine"] = round(rec["fetch_fraction"] / cal, 4)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
