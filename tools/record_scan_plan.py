#!/usr/bin/env python3
"""Record the scan plan of every row of tests/plan_cases.py into tests/golden/scan_plan.json (or --out FILE): the kernel's name, the
launch / stream / window counts and what the prefilter did, with the device's compute-unit count.  tests/test_gpu_scan_plan.py
holds the library to this record, so it is made on the commit whose plan is to be kept: build that commit, run this once on the
MI355X, commit the file.

Every row runs in a child process of its own under a time limit; the first row that fails ends the run and nothing is written.
With KGMA_GEOM_DEBUG=1 in the environment the library's geometry lines go to stderr, each row's behind a `== row` line: the stderr
of two builds can be compared with diff."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kmergma.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROW_TIMEOUT_S = 120


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scan_plan.json"))
    ap.add_argument("--row", help="run this row alone and print its record (what the recorder's child processes do)")
    args = ap.parse_args()
    from tests import plan_cases as pc
    if args.row:
        print(json.dumps(pc.run_case(args.row)))
        return 0
    import torch
    out = {"compute_units": int(torch.cuda.get_device_properties(0).multi_processor_count), "cases": {}}
    for name in pc.CASES:
        sys.stderr.write(f"== {name}\n")
        sys.stderr.flush()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name], stdout=subprocess.PIPE, timeout=ROW_TIMEOUT_S, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"row {name} failed with status {r.returncode}: nothing written\n")
            return 1
        out["cases"][name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, json.dumps(out["cases"][name]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
