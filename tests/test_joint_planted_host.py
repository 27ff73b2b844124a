"""``HostJointState`` -- the numpy statement every CPU run and every device test of the joint state leans on -- against
the brute-force reference of joint_planted_support.py, on planted (live, shelf) pairs.  In a consistent run the purge of
``prepare`` never drops an entry, so the statement itself had never seen a drop.  Also here, on the reference alone:
that the generated cases contain what they are for.  Needs no device."""
import pytest

import joint_planted_support as jp

PREPARE_CASES = jp.prepare_cases()
DENSE_CASES = jp.dense_cases()


@pytest.mark.parametrize("case", PREPARE_CASES, ids=[c["name"] for c in PREPARE_CASES])
def test_host_prepare_on_planted_states(case):
    nlive, ndata = case["live"].shape
    seen = jp.new_seen()
    jp.run_prepare_case(jp.HostDriver(nlive, ndata), case, seen)
    assert seen["drops"], "the case planted nothing"


@pytest.mark.parametrize("case", DENSE_CASES, ids=[c["name"] for c in DENSE_CASES])
def test_host_chunks_on_planted_states(case):
    nlive, ndata = case["live"].shape
    jp.run_dense_case(jp.HostDriver(nlive, ndata), case)


def test_the_prepare_cases_contain_what_they_are_for():
    """Every drop pattern, tie pair, special column, threshold position, shelf length and running-list length occurs,
    every planting chunk accepts candidate 0 with the intended bits and every shelf reaches its length (asserted in
    ``plant``) -- by the reference alone."""
    seen = jp.new_seen()
    for case in PREPARE_CASES:
        ref = jp.run_prepare_case(None, case, seen)
        assert ref.sizes()[ref.running].sum() == 0
        # a state made with room for 4 doubles its shelves whenever the longest is full: what the device must report
        longest = max(len(s) for s in case["shelves"])
        assert case["cap"] == max(4, 1 << (longest - 1).bit_length())
    jp.check_prepare_coverage(seen)
    assert "first128" in seen["drops"], "no case had w_held == 0 with survivors beyond entry 128"
    assert any(case["cap"] == 256 for case in PREPARE_CASES)


def test_the_dense_cases_contain_what_they_are_for():
    seen = set()
    for case in DENSE_CASES:
        seen |= jp.run_dense_case(None, case).seen
    jp.check_dense_coverage(seen)
