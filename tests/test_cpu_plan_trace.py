"""The launch sequence of UNetPlan — every call, descriptor field, buffer size, offset and aliasing of a forward pass, a
training step and an inference tile — against the recorded hashes (tests/plan_trace.py; no device is used).  The hashes
were recorded before the plan's builders were folded: a refactor of the plan keeps every one of them."""

import json

import pytest

import plan_trace


@pytest.fixture(scope="module")
def traces():
    with pytest.MonkeyPatch.context() as mp:            # (undone on exit: no stub and no switch is left behind)
        return plan_trace.all_traces(mp)


def test_launch_traces_match_the_recorded_hashes(traces):
    with open(plan_trace.HASHES) as f:
        want = json.load(f)
    assert sorted(traces) == sorted(want)
    moved = [key for key, text in traces.items() if plan_trace.digest(text) != want[key]]
    assert not moved, ("launch traces changed: %s — `python tests/plan_trace.py --dump DIR` on both trees and diff the "
                       "text files of these ids" % moved)


def test_every_switch_moves_a_trace(traces):
    """a switch of the matrix that changes no trace pins nothing (CLX_CHAIN64=0 is the deterministic plans' state, so
    it is compared with the default plans only)"""
    for env in list(plan_trace.ENVS)[1:] + list(plan_trace.TRAIN_ENVS):
        assert any(text != traces[key.rsplit("/", 1)[0] + "/default"] for key, text in traces.items()
                   if key.endswith("/" + env)), env


# (entry point, argument position) that may take an address outside the plan's storages: the caller's tensor made
# contiguous, a weight copied with gaps for a concatenation of odd channel counts (_expand_cin), and that copy's
# counterpart on the way back (the temporary of _unpack_step, which torch ops then compress into the gradient)
TEMPORARIES = {("clx_planar_to_pixel", 1), ("clx_pack_weights", 1), ("clx_subpixel_split_weights", 1), ("clx_unpack_wgrad", 2)}


def test_descriptors_point_into_the_plans_storages(traces):
    for key, text in traces.items():
        for line in text.splitlines()[9:]:
            words = line.split(" ")
            for i, w in enumerate(words):
                if "?" in w:
                    assert (words[0], i) in TEMPORARIES and w.startswith("?"), (key, line)
