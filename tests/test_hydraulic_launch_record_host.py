"""The Python launch path of ``HydraulicNetwork``, held to a record: tests/golden/hydraulic_launches.json lists, for every level of
``simulate`` and ``simulate_series``, every optional array per launch and per scenario, every refusal, the draws and the two store
generators, each native launch with its entry point, its scalars and what every pointer points to, and the result's class, dtypes
and shapes.  tests/golden/make_hydraulic_launches.py records it without a device (a fake library, networks on the CPU) and says
what an entry means; the file was recorded before the launch path was restated once, so the restatement launches what the ladder
launched."""
import importlib.util
import json
import os

import pytest

import gnn_pressure_estimation_amd as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def records():
    spec = importlib.util.spec_from_file_location("make_hydraulic_launches", os.path.join(GOLDEN, "make_hydraulic_launches.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(maker.PATH) as f:
        want = json.load(f)
    got = json.loads(maker.dumps(maker.record(G)))          # (through JSON: tuples become lists, as in the file)
    return want, got


def test_the_record_has_the_cases_of_the_file_in_its_order(records):
    want, got = records
    assert list(got) == list(want) and len(want) >= 200


def test_every_launch_has_the_argument_count_of_its_signature(records):
    _, got = records
    launches = [c for case in got.values() for c in case["launches"]]
    assert len(launches) > 300
    for name, count, args in launches:
        assert count == len(args) == len(G._native.SIGNATURES[name][1]), name


def test_every_case_launches_what_the_file_records(records):
    want, got = records
    for name in want:
        assert len(got[name]["launches"]) == len(want[name]["launches"]), name
        for mine, theirs in zip(got[name]["launches"], want[name]["launches"]):
            assert mine[:2] == theirs[:2], name
            for k, (a, b) in enumerate(zip(mine[2], theirs[2])):
                assert a == b and type(a) is type(b), (name, mine[0], k)


def test_every_case_returns_or_refuses_what_the_file_records(records):
    want, got = records
    for name in want:
        assert {k: v for k, v in got[name].items() if k != "launches"} == {k: v for k, v in want[name].items() if k != "launches"}, name
