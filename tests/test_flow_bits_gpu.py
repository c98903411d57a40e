"""GPU: the flow handle gives the bits it gave before its host half was reorganised (csrc/vq_flow.hip, csrc/host/vq_flow_host.cc).

tests/golden/flow_plan/parent_bits.json holds sha256 hashes (and the integer counts) of what the commit BEFORE that change returned on
the cases of tests/_flow_bits_cases.py, recorded on an MI355X by tools/flow_record_bits.py in two runs that agreed; this tree must
return the same bytes.  The cases: (A) a plain flow whose iteration count is no multiple of the block and whose levels are ragged, (B)
the same through three homographies, (C) the stop rule live on six pairs, (D) vq_flow_warped on the guard batch, (E) the corner search
and the RANSAC with refit on their own.  H is compared as the bytes of its doubles: it passes through the host's fp64 algebra.
tests/golden/flow_plan/tile_cuts.json: the cuts the same commit named for 1..32 pairs on seven shapes, which depend on the device's
compute units and are compared on a device with as many."""
import json
import os

import pytest

import _flow_bits_cases as bc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_plan")


@pytest.fixture(scope="module")
def flow_mod(gpu):
    from video_query_algorithms_amd.tsn import flow
    return flow


@pytest.fixture(scope="module")
def parent_bits():
    with open(os.path.join(GOLDEN, "parent_bits.json")) as f:
        return json.load(f)


def test_every_case_was_recorded(parent_bits):
    assert set(parent_bits) == set(bc.CASES)
    assert set(parent_bits["A"]) == set(parent_bits["B"]) == set(parent_bits["C"]) == set(bc.FLOW_KEYS)
    assert set(parent_bits["D"]) == set(bc.WARPED_KEYS) and set(parent_bits["E_ransac"]) == {"H", "inliers", "winner", "mask"}
    assert parent_bits["A"]["iters"]["values"] == [9] * 18 and parent_bits["A"]["u1"]["shape"] == [3, 61, 83]
    assert len(set(parent_bits["C"]["iters"]["values"])) == 6 and max(parent_bits["C"]["iters"]["values"]) == 48       # the stop rule acted
    assert parent_bits["D"]["matches"]["values"][1] == 0 and parent_bits["D"]["inliers"]["values"][0] > 25              # (b) flat, (a) camera motion


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_same_bits_as_before_the_reorganisation(flow_mod, parent_bits, name):
    got = bc.record(bc.CASES[name](flow_mod))
    want = parent_bits[name]
    assert set(got) == set(want)
    for key in sorted(want):
        assert got[key] == want[key], "case %s, %s: %s, recorded %s" % (name, key, got[key], want[key])


def test_tile_cuts_are_the_recorded_ones(flow_mod):
    import torch
    with open(os.path.join(GOLDEN, "tile_cuts.json")) as f:
        recorded = json.load(f)
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    if slots != recorded["slots"]:
        pytest.skip("the cuts were recorded on %d workgroup slots, this device has %d" % (recorded["slots"], slots))
    assert bc.tile_cuts(flow_mod) == recorded["shapes"]
