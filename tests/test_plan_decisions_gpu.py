"""The decisions of device plans — engines, workspace, and which engine and sort serve five fixed point sets — pinned for a matrix of
193 plans on the MI355X (tests/golden/plan_decisions_gpu.json, recorded by scripts/plan_decisions.py with the library of the commit before
the decisions moved into csrc/plan_engines.cpp)."""
import json
import os

import pytest

from test_plan_decisions_host import ROOT, assert_same_records, load_tool


@pytest.mark.gpu
def test_device_plans_decide_what_the_recorded_ones_did():
    tool = load_tool()
    with open(os.path.join(ROOT, "tests", "golden", "plan_decisions_gpu.json")) as f:
        golden = json.load(f)
    cus = tool.num_cus(0)
    if cus != golden["num_cus"]:
        pytest.skip(f"recorded on a device of {golden['num_cus']} compute units, this one has {cus}: the launch models differ")
    doc = tool.snapshot(0)
    assert doc["info_fields"] == golden["info_fields"] and doc["set_fields"] == golden["set_fields"]
    assert len(doc["plans"]) == 193
    assert_same_records(tool, golden, doc)
