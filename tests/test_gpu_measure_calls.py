"""The measure and relate stages' library calls and results on small formula-made inputs -- every flag of region_table alone
and all together, 2-D, 3-D and maps without objects, the other entry points -- against the record in tests/measure_calls.json
(tests/measure_calls.py).  The record was made before the stage's host code was restructured: a refactor of the stage keeps
every entry, call for call and byte for byte."""

import json

import pytest

import measure_calls


@pytest.mark.gpu
def test_calls_and_results_match_the_record(device):
    got = measure_calls.compacted(measure_calls.all_records(device))
    with open(measure_calls.RECORD) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    moved = [f"{key} ({part})" for key in want for part in ("calls", "result") if got[key][part] != want[key][part]]
    assert not moved, ("the stage's calls or results changed: %s -- `python tests/measure_calls.py --dump DIR` on both trees and "
                       "diff the text files of these ids" % moved)
