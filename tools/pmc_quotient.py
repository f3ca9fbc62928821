"""Summarise the counters-only rocprofv3 passes of tools/pmc_quotient.sh: per quotient row kernel
(name, field, Montgomery or canonical) the mean of every counter over the kernel's dispatches, one
JSON line per kernel. Each pass directory holds one counter set, so a counter's mean is taken over
the dispatches of its own pass.
Usage: python3 tools/pmc_quotient.py <dir holding the pass directories>"""
import collections
import csv
import glob
import json
import re
import sys


def main():
    root = sys.argv[1]
    agg = collections.OrderedDict()
    for f in sorted(glob.glob(root + "/**/*counter_collection.csv", recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"(quot_\w+)<b2f::field::(\w+)(?:, (\w+))?>", r["Kernel_Name"])
                if not m or m.group(1) in ("quot_consts_kernel", "quot_gate_consts_kernel"):
                    continue
                key = (m.group(1), m.group(2).lower(), m.group(3) or "")
                d = agg.setdefault(key, collections.defaultdict(list))
                d[r["Counter_Name"]].append(float(r["Counter_Value"]))
                d["scratch"] = [float(r["Scratch_Size"])]
    for (name, field, mont), d in agg.items():
        rec = {"kernel": name, "field": field, "montgomery": mont}
        rec.update({k: round(sum(v) / len(v), 1) for k, v in sorted(d.items())})
        rec["dispatches"] = max(len(v) for v in d.values())
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
