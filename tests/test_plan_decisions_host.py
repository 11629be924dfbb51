"""Every decision of plan creation that needs no device, pinned for a fixed matrix of about 1650 host-only plans.

tests/golden/plan_decisions_host.json was recorded by scripts/plan_decisions.py with the library of the commit before the decisions
moved into csrc/plan_engines.cpp; a change that is meant to preserve behaviour must reproduce it field by field."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("plan_decisions", os.path.join(ROOT, "scripts", "plan_decisions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_same_records(tool, golden, doc):
    """equality of every field of every record, with a readable report of the first differences"""
    keys = list(doc["plans"])
    assert len(keys) == golden["matrix"]["plans"] and tool.matrix_digest(keys) == golden["matrix"]["sha256"], "the matrix of plans differs from the recorded one"
    diffs = []
    for key, want, rec in zip(keys, tool.decode(golden), doc["plans"].values()):
        got = tool.flatten(doc, rec)
        if got != want:
            what = [f"{c} = {got.get(c)!r} instead of {want.get(c)!r}" for c in dict.fromkeys(list(want) + list(got)) if got.get(c) != want.get(c)]
            diffs.append(f"{key}: " + "; ".join(what))
    assert not diffs, f"{len(diffs)} of {len(keys)} plans differ:\n" + "\n".join(diffs[:40])


def test_host_plans_decide_what_the_recorded_ones_did():
    tool = load_tool()
    with open(os.path.join(ROOT, "tests", "golden", "plan_decisions_host.json")) as f:
        golden = json.load(f)
    doc = tool.snapshot(-1)
    assert doc["info_fields"] == golden["info_fields"] and doc["real_fields"] == golden["real_fields"]
    assert len(doc["plans"]) >= 1600
    assert_same_records(tool, golden, doc)
