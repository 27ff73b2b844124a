"""The joint state on the device (csrc/mdns_joint.hip) on PLANTED states: ``k_joint_prepare`` as a function of (live,
shelf, running) -- the purge that drops entries, which no consistent run ever reaches, lane, register and keep-word
edges, ties, +-inf --, ``k_joint_accept_dense`` / ``k_joint_commit_dense`` (``shelf_append``, ``first_flagged``) on
likelihoods that sit exactly on, one ulp above and far from their thresholds, and ``mdns_joint_undo_advance_dev``.

Every likelihood is planted bit for bit (joint_planted_support.py says how), the reference is brute-force numpy, and
every comparison is exact.  That the cases contain what they are for is asserted on the reference alone in
test_joint_planted_host.py, which runs without a device."""
import numpy as np
import pytest

import joint_planted_support as jp

pytestmark = pytest.mark.gpu

PREPARE_CASES = jp.prepare_cases()
DENSE_CASES = jp.dense_cases()


@pytest.mark.parametrize("case", PREPARE_CASES, ids=[c["name"] for c in PREPARE_CASES])
def test_prepare_on_planted_states(case):
    """Planting (every chunk accepts candidate 0 with the intended bits; the shelves grow 4 -> ``case["cap"]``), the live
    matrix overwritten in place, then the call under test: Lmin, argmin, raw keep words, thresholds and shelf sizes of
    all data sets -- the ones that do not run unchanged -- and the purged shelves read out in order by advance ->
    get_live -> prepare on a running list that shrinks as they run empty."""
    nlive, ndata = case["live"].shape
    driver = jp.DeviceDriver(nlive, ndata, shelf_cap=4)
    try:
        seen = jp.new_seen()
        jp.run_prepare_case(driver, case, seen)
        assert seen["drops"] and seen["nrun"]
    finally:
        driver.close()


@pytest.mark.parametrize("nlive", [17, 129])
def test_prepare_of_the_state_object_decodes_the_keep_words(nlive):
    """What the sampler consumes: ``prepare`` of the Python state turns the keep words into the bool matrix
    ``keep[r, e]``, as wide as the longest shelf of the running data sets, and counts what stays."""
    case = jp.case_small(nlive)
    driver = jp.DeviceDriver(nlive, case["live"].shape[1], shelf_cap=4)
    try:
        ref = jp.planted_state(driver, case)
        lengths = ref.sizes()[ref.running]
        Lmin, arg, keep = driver.js.prepare()
        want = ref.prepare()
        assert np.array_equal(Lmin, want[0]) and np.array_equal(arg, want[1])
        matrix = np.zeros((len(ref.running), lengths.max()), dtype=bool)
        for r, k in enumerate(want[2]):
            matrix[r, :len(k)] = k
        assert matrix.sum(axis=1).tolist() != lengths.tolist(), "the case drops nothing"
        assert keep is not None and np.array_equal(keep, matrix)
        assert np.array_equal(driver.js.shelf_n[ref.running], matrix.sum(axis=1))
        jp.same_state(driver, ref, "decoded prepare")
    finally:
        driver.close()


@pytest.mark.parametrize("case", DENSE_CASES, ids=[c["name"] for c in DENSE_CASES])
def test_dense_chunks_on_planted_states(case):
    """Per chunk of ``jp.DENSE_CHUNKS``: the accepted index (the lowest acceptable candidate; -1 and nothing changed
    where nobody is), the raw fill words (bits at and beyond M zero), thresholds and shelf sizes of ALL data sets."""
    nlive, ndata = case["live"].shape
    driver = jp.DeviceDriver(nlive, ndata, shelf_cap=4)
    try:
        ref = jp.run_dense_case(driver, case)
        assert ref.seen
    finally:
        driver.close()


def test_undo_advance_restores_the_live_matrix():
    """What bench.py relies on between repetitions: after prepare, draws and advance on a running subset,
    mdns_joint_undo_advance_dev gives back the live matrix of before the advance and empties the running shelves;
    data sets that do not run keep live values, shelves and thresholds."""
    nlive, ndata = 17, 70
    rng = np.random.RandomState(17)
    case = {"name": "undo", "live": rng.randint(0, 30, size=(nlive, ndata)).astype(np.float64),
            "shelves": [40.0 + np.arange(d % 3) for d in range(ndata)], "running": np.flatnonzero(np.arange(ndata) % 4 != 1), "cap": None}
    driver = jp.DeviceDriver(nlive, ndata, shelf_cap=4)
    try:
        ref = jp.planted_state(driver, case)
        running = ref.running
        idle = np.setdiff1d(np.arange(ndata), running)
        jp.compare_prepare(driver, ref, "undo")
        for k in range(2):                                 # one more entry on every running shelf, then on every other
            rows = running[::k + 1].astype(np.int32)
            L = np.nextafter(ref.higher[rows], np.inf).reshape(1, -1)
            idx, beats = jp.compare_chunk(driver, ref, L, rows, "undo")
            assert idx == 0 and beats.all()
        before = driver.live_matrix()
        higher, sizes = driver.thresholds()
        assert (sizes[running] >= 1).all() and (sizes[idle] > 0).any()
        ref.advance()
        driver.advance()
        moved = driver.live_matrix()
        assert np.array_equal(moved, ref.live) and (moved[:, running] != before[:, running]).any(axis=0).all()
        driver.undo_advance()
        assert np.array_equal(driver.live_matrix(), before)
        higher2, sizes2 = driver.thresholds()
        assert (sizes2[running] == 0).all()
        assert np.array_equal(sizes2[idle], sizes[idle]) and np.array_equal(higher2[idle], higher[idle])
        # the iteration runs again from there, as the benchmark's repetitions do
        ref.live = before.copy()
        for d in running:
            ref.shelf[d] = np.zeros(0)
        jp.compare_prepare(driver, ref, "after undo")
    finally:
        driver.close()
