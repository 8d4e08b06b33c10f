#!/usr/bin/env python3
"""Per-launch MEDIANS of rocprofv3 counters for the rt_trace kernels, one line per pass directory.

    python3 profiles/pmc_medians.py <dir>      reads every <dir>/pmc_<name>/**/*counter_collection.csv, where each pmc_<name> is the
                                               output directory (-d) of one `rocprofv3 --pmc <counters> --output-format csv -- bench.py ...`
                                               pass (counters in passes of their own, never with tracing)

The median leaves out the few launches of a bench run that are not the timed ones (the first frame from a camera: four-wave
workgroups, one workgroup per block), where run_profile.sh's summaries average.  Used for A/B libraries (RT_HIP_LIB) whose passes
are named by the caller: profiles/uniform_blocks_counters*.txt.
"""
import collections
import csv
import glob
import os
import sys

root = sys.argv[1]
for d in sorted(glob.glob(os.path.join(root, "pmc_*"))):
    if not os.path.isdir(d):
        continue
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                k = row.get("Kernel_Name", "")
                if "rt_trace" not in k:
                    continue
                acc[k[:60]][row["Counter_Name"]].append(float(row["Counter_Value"]))
    for k, cs in acc.items():
        out = {c: sorted(v)[len(v) // 2] for c, v in cs.items()}
        n = {c: len(v) for c, v in cs.items()}
        print(os.path.basename(d), k, {c: int(x) for c, x in out.items()}, "launches", max(n.values()))
