#!/usr/bin/env python3
"""Record the scan plan of every row of tests/plan_cases.py into tests/golden/scan_plan.json (or --out FILE): the kernel's name, the
launch / stream / window counts and what the prefilter did, for the chain replay rows what the replay selected, where its chains ran
and a digest of the hits, for the chain_export rows the pair's stream layout, with the device's compute-unit count.
tests/test_gpu_scan_plan.py holds the library to this record, so it is made on the commit whose plan is to be kept: build that
commit, run this once on the MI355X, commit the file.

Every row runs in a child process of its own under a time limit; the first row that fails ends the run and nothing is written.
A replay row that selects no chain pair (or too few, or chains them in the wrong place) pins nothing: the run goes on, to name every
such row, and nothing is written.  A chain_export row runs twice: the pool's unit count is recorded only where both runs agree on it.
With KGMA_GEOM_DEBUG=1 / KGMA_CHAIN_DEBUG=1 in the environment the library's geometry / chain lines go to stderr, each row's behind
a `== row` line: the stderr of two builds can be compared with diff."""
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

    def run_row(name):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name], stdout=subprocess.PIPE, timeout=ROW_TIMEOUT_S, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"row {name} failed with status {r.returncode}: nothing written\n")
            return None
        return json.loads(r.stdout.strip().splitlines()[-1])

    unpinned = 0
    for name in pc.CASES:
        sys.stderr.write(f"== {name}\n")
        sys.stderr.flush()
        got = run_row(name)
        if got is None:
            return 1
        if "export" in got:
            again = run_row(name)
            if again is None:
                return 1
            if again["export"]["pool_units"] != got["export"]["pool_units"]:
                sys.stderr.write(f"row {name}: pool of {got['export']['pool_units']} units, then {again['export']['pool_units']}: left out\n")
                del got["export"]["pool_units"]
        err = pc.chain_row_error(name, got)
        if err:
            sys.stderr.write(f"row {name}: {err}\n")
            unpinned += 1
        out["cases"][name] = got
        print(name, json.dumps(got), flush=True)
    if unpinned:
        sys.stderr.write(f"{unpinned} chain row(s) pin nothing: nothing written\n")
        return 1
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
