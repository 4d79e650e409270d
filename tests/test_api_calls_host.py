"""CPU tier of loam_livox_amd/api.py as a marshalling layer: every public method, driven once over the recording stand-in
(tests/api_calls_driver.py on tests/api_standin.py), makes the C calls -- names, order, every argument down to the bytes of the arrays --
and returns the values that tests/api_calls.json holds.  The file was written by the same driver at a3c4a91, before api.py's idioms
became helpers (the driver's docstring says how), so the comparison is with what each method did then.

One case differs on purpose and says so here, not in the recording: History_buffer.map_cloud raises when the library answers a negative
count, as History_buffer_batch.map_cloud always did; at a3c4a91 it returned an empty cloud."""
import json
import os

import pytest

from loam_livox_amd import capi
from tests import api_calls_driver as driver

RECORDED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "api_calls.json")))
MAP_CLOUD_CASE = "history_buffer_map_cloud_negative"


def test_the_recording_holds_the_driver_s_cases():
    assert sorted(RECORDED) == sorted(driver.CASES)
    for name, rec in RECORDED.items():
        assert rec["calls"], name


@pytest.mark.parametrize("case", [c for c in driver.CASES if c != MAP_CLOUD_CASE])
def test_calls_and_returns_are_the_recorded_ones(monkeypatch, case):
    got = driver.run(case, lambda lib: monkeypatch.setattr(capi, "_lib", lib))
    want = RECORDED[case]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i} ({w[0]})"
    assert len(got["returns"]) == len(want["returns"])
    for i, (g, w) in enumerate(zip(got["returns"], want["returns"])):
        assert g == w, f"return value {i}"


def test_map_cloud_with_a_negative_count_is_the_one_difference(monkeypatch):
    got = driver.run(MAP_CLOUD_CASE, lambda lib: monkeypatch.setattr(capi, "_lib", lib))
    want = RECORDED[MAP_CLOUD_CASE]
    assert want["returns"] == [{"dtype": "float32", "shape": [0, 4], "bytes": ""}]   # then: an empty cloud
    assert got["returns"] == [{"raises": "LoamLivoxError"}]                            # now: the library's error
    # the same calls, and the question for the error text where the empty cloud was made
    size_call = ["ll_history_map_cloud", [{"pointer": 0x1000}, 0, None, 0]]
    assert size_call in want["calls"]
    assert got["calls"] == want["calls"][:want["calls"].index(size_call) + 1] + [["ll_last_error", []]] + want["calls"][want["calls"].index(size_call) + 1:]
