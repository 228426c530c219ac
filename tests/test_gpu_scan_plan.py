"""The scan plan is what tests/golden/scan_plan.json recorded (tools/record_scan_plan.py): for every row of tests/plan_cases.py the
kernel's name, the number of launches and streams, the bases and windows scanned, the dip / hit / at-threshold counts and what the
prefilter did; for the chain replay rows also what the replay selected, where its chains ran and a digest of the hit list; for the
chain_export rows the stream layout of the pair.  The parity tests pin results and leave the plan loose (kernel_name().startswith(...)); a change that moves a
configuration to another correct kernel, regroups its launches or resizes its streams keeps them green and changes the speed.

The number of streams (stats n_tiles, the filter's streams) follows from the device's compute-unit count: those two fields are
compared only on a device with the recorded count, every other field always (plan_cases.cu_fields)."""
import json
import os
import subprocess
import sys

import pytest

from tests import plan_cases as pc
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "scan_plan.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def same_device(recorded):
    """The device's compute-unit count, as the recorder reads it -- asked once, in a process of its own: torch brings a HIP runtime
    of its own, which finds no device in a process where the library's runtime already holds it."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    return int(out.stdout.split()[-1]) == recorded["compute_units"]


def test_every_row_is_recorded(recorded):
    assert sorted(recorded["cases"]) == sorted(pc.CASES)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_scan_plan(recorded, same_device, name):
    want, got = recorded["cases"][name], pc.run_case(name)
    print(name, json.dumps(got))
    assert sorted(got) == sorted(want)
    if "export" in want:
        for f in pc.EXPORT_FIELDS + (("pool_units",) if "pool_units" in want["export"] else ()):
            assert got["export"][f] == want["export"][f], (name, f, got["export"][f], want["export"][f])
        return
    assert got["kernel"] == want["kernel"]
    for part, fields in (("stats", pc.STATS_FIELDS), ("filter", pc.FILTER_FIELDS), ("chain", pc.CHAIN_FIELDS)):
        if part not in want:
            continue
        for f in fields:
            if f in pc.cu_fields(name, part) and not same_device:
                continue
            assert got[part][f] == want[part][f], (name, part, f, got[part][f], want[part][f])
    assert pc.chain_row_error(name, got) is None
    assert got.get("hits_sha256") == want.get("hits_sha256")
