"""Summarise `rocprofv3 --pmc ... --output-format csv` passes of `profiles/kslots_wide_bench.py` per kernel and per SLOT: the
K-slot kernel's counters divided by its 25 slots against the three launches of a one-slot slot (step, driver_shape,
sps_step_wave).  Usage: python profiles/kslots_wide_pmc.py <dir with the passes' *counter_collection.csv> ..."""
import collections
import csv
import glob
import re
import sys

K = 25


def main():
    files = []
    for d in sys.argv[1:]:
        files += glob.glob(d + "/**/*counter_collection.csv", recursive=True)
    # (kernel, grid) -> counter -> per-dispatch values
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in files:
        for r in csv.DictReader(open(f)):
            name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "")
            if not any(s in name for s in ("step_wide", "sps_step_wave", "driver_shape")):
                continue
            key = (name, int(r.get("Grid_Size", 0) or 0))
            agg[key][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("per dispatch means; 'per slot' = / %d for step_wide_slots_kernel, as is for the one-slot kernels" % K)
    for (name, grid), d in sorted(agg.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        div = K if "slots" in name else 1
        vals = {c: sum(v) / len(v) / div for c, v in d.items()}
        n = max(len(v) for v in d.values())
        print("%-70s grid %9d  dispatches %3d  per slot: %s" % (name[:70], grid, n,
              "  ".join("%s %.4g" % (c, v) for c, v in sorted(vals.items()))))


if __name__ == "__main__":
    main()
