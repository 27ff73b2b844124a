"""The grouping kernels (csrc/mdns_groups.hip) at the edges of their own geometry, against scipy's connected
components and numpy.unique (groups_support.py): the one-workgroup compaction where a thread lists more than one
word and at its scan's wave boundaries, the rounds where a wave strides over its ids more than once and the last
workgroup is not full, the outputs no other test compares (bit map of a subset, -1 point labels, labels at size),
sequences on one handle whose state must not leak, deferred and immediate refusals, the stamps starting over, and
the sampler core's device branch on planted matrices.  Integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib
from groups_support import (STAMP_WRAP, check_call, compact_run, cpu_point_labels, debug_set_call, dense_matrix, embed,
                            family_matrix, fill_columns, random_matrix, raw_components, set_ids, shuffled_path,
                            sparse_edge_ids)
from test_groups import clustered_ids, cpu_groups, same

pytestmark = pytest.mark.gpu

#: nwords 1 ... 1024 (run 1, all threads busy at 65 536), 1025 (run 2, threads from 513 on idle), 2049 (run 3),
#: 4688 (run 5, a partial last run)
LADDER = (1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 131072, 131073, 300001)
FAMILIES = ("disjoint", "bridge", "path", "clustered")


def _groups(lp):
    from massivedatans_amd.grouping import DeviceGroups
    return DeviceGroups(lp)


def _subset(ndata, leave_every=3):
    rows = np.flatnonzero(np.arange(ndata) % leave_every != 1)
    return rows if len(rows) else np.arange(ndata)


# ---------------------------------------------------------------------------------- A. compaction and bit map

def test_ladder_geometry():
    """The sizes of the ladder reach what they are there for (k_groups_compact: 1024 threads)."""
    assert [compact_run(n) for n in (65536, 65537, 131072, 131073, 300001)] == [1, 2, 2, 3, 5]
    assert (300001 + 63) // 64 == 4688 and 4688 % 5 != 0
    assert sparse_edge_ids(1).tolist() == [0]
    assert {0, 63, 64, 127, 63 * 64, 64 * 64 - 1, 64 * 64, 65 * 64 - 1, 65535} <= set(sparse_edge_ids(65536).tolist())
    assert {0, 4 * 64, 5 * 64 - 1, 5 * 64, 6 * 64 - 1, 512 * 5 * 64, 300000} <= set(sparse_edge_ids(300001).tolist())


@pytest.mark.parametrize("pattern", ["sparse", "dense", "random"])
def test_compaction_ladder_on_one_handle(pattern):
    """One handle walks the ladder upwards -- its per-id block and its box of distinct ids grow several times,
    4096 -> 524 288 -- with the ids at the compaction's hand-over points, with every id held, with about 30 %
    held; all data sets and a subset; then back to 4097 points with all ids below that: nothing of the large
    calls may show."""
    rng = np.random.RandomState(len(pattern))
    nlive, ndata = {"sparse": (2, 16), "dense": (100, 1311), "random": (100, 1000)}[pattern]
    ladder = [n for n in LADDER if pattern != "dense" or n <= 131073]

    def matrix(npoints):
        if pattern == "sparse":
            return fill_columns(sparse_edge_ids(npoints), nlive, ndata)
        if pattern == "dense":
            return dense_matrix(npoints, nlive, ndata)
        return random_matrix(rng, npoints, nlive, ndata)

    dg = _groups(matrix(ladder[0]))
    for npoints in ladder + [4097]:
        lp = matrix(npoints)
        set_ids(dg, lp)
        assert np.array_equal(dg.ids(), lp)
        check_call(dg, lp, None, npoints)
        if pattern == "dense":
            ncomp, ids = dg.components(None, npoints)
            assert len(ids) == npoints                       # every id held
        check_call(dg, lp, _subset(ndata), npoints)
    # ... and the same after a replacement instead of a whole new matrix: ids near the top leave, low ones come
    rows = np.arange(0, ndata, 2)
    slots = np.arange(len(rows)) % nlive
    new = np.arange(len(rows)) % 64
    lp[slots, rows] = new
    dg.replace(rows, slots, new)
    check_call(dg, lp, None, 4097)
    dg.close()


# ---------------------------------------------------------------------------------- B. wave geometry

@pytest.mark.parametrize("nlive", [1, 2, 63, 64, 65, 127, 128, 129, 200])
def test_round_geometry(nlive):
    """k_groups_round: one wave per data set, four per workgroup, lanes striding the ids by 64.  Every number
    of selected data sets around the workgroup size and beyond one wave of waves, as the whole matrix and as
    subsets of a larger one whose other columns would join everything; four graph families each."""
    rng = np.random.RandomState(1000 + nlive)
    one = several = cases = 0
    many_disjoint = False
    for M in (1, 2, 3, 4, 5, 7, 8, 9, 257):
        every4 = np.arange(0, 4 * M - 3, 4)
        skip = M // 2
        but_one = np.delete(np.arange(M + 1), skip)
        handles = [_groups(np.zeros((nlive, nd), dtype=np.int64)) for nd in (M, 4 * M - 3, M + 1)]
        for family in FAMILIES:
            lp, npoints = family_matrix(rng, family, nlive, M)
            want = cpu_groups(lp, np.arange(M))
            if family == "disjoint":
                assert len(want) == M
            counts = []
            # the whole matrix
            set_ids(handles[0], lp)
            counts.append(check_call(handles[0], lp, None, npoints, want))
            # every 4th of 4 M - 3, and its first and last data set alone
            big = embed(rng, lp, npoints, every4, 4 * M - 3)
            set_ids(handles[1], big)
            counts.append(check_call(handles[1], big, every4, npoints))
            counts.append(check_call(handles[1], big, every4[:1], npoints))
            counts.append(check_call(handles[1], big, every4[-1:], npoints))
            # all but one of M + 1
            big = embed(rng, lp, npoints, but_one, M + 1)
            set_ids(handles[2], big)
            counts.append(check_call(handles[2], big, but_one, npoints))
            assert counts[0] == counts[1] == counts[4] == len(want) and counts[2] == counts[3] == 1
            cases += len(counts)
            one += sum(c == 1 for c in counts)
            several += sum(c > 1 for c in counts)
            many_disjoint = many_disjoint or (family == "disjoint" and M > 64 and counts[0] == M)
        for dg in handles:
            dg.close()
    assert 3 * one >= cases and 3 * several >= cases and many_disjoint


@pytest.mark.parametrize("nlive", [31, 32, 33, 65])
@pytest.mark.parametrize("ndata", [31, 32, 33, 65])
def test_transpose_tiles(nlive, ndata):
    """k_groups_transpose (32 x 32 tiles) on both sides of a tile edge, there and back, and k_groups_replace at
    the corners of the matrix."""
    rng = np.random.RandomState(nlive * 100 + ndata)
    lp = rng.randint(0, 5000, size=(nlive, ndata)).astype(np.int64)
    dg = _groups(lp)
    assert np.array_equal(dg.ids(), lp)
    for rows, slots in (([0, ndata - 1], [0, nlive - 1]), ([0, ndata - 1], [nlive - 1, 0])):
        new = rng.randint(5000, 6000, size=2)
        lp[slots, rows] = new
        dg.replace(rows, slots, new)
        assert np.array_equal(dg.ids(), lp)
    lp2 = rng.randint(0, 5000, size=(nlive, ndata)).astype(np.int64)
    set_ids(dg, lp2)
    assert np.array_equal(dg.ids(), lp2)
    check_call(dg, lp2, None, 5000)
    dg.close()


# ---------------------------------------------------------------------------------- C. sequences on one handle

def test_stale_stamps_of_the_other_selection():
    """Selections A and B share no id: what A's call stamped is one call old when B's runs -- the case the
    stamps exist for.  300 calls alternately, a replacement every 10th; counts on every call, everything on
    every 25th."""
    rng = np.random.RandomState(3)
    nlive, half, span = 8, 32, 300
    lp = np.concatenate([clustered_ids(rng, nlive, half, 3, 60), span + clustered_ids(rng, nlive, half, 4, 60)], axis=1)
    npoints = 2 * span
    sels = (np.arange(half), half + np.arange(half))
    dg = _groups(lp)
    want = [None, None]
    for it in range(300):
        which = it % 2
        if it % 10 == 9:
            rows = np.flatnonzero(rng.uniform(size=2 * half) < 0.3)
            slots = rng.randint(0, nlive, size=len(rows))
            new = (rows >= half) * span + rng.randint(0, span, size=len(rows))     # each side keeps to its own ids
            lp[slots, rows] = new
            dg.replace(rows, slots, new)
            want = [None, None]
        if want[which] is None:
            want[which] = cpu_groups(lp, sels[which])
        ncomp, ids = dg.components(sels[which], npoints)
        assert ncomp == len(want[which])
        assert len(ids) == sum(len(p) for _, p in want[which])
        if it % 25 == 0 or it % 25 == 24:                   # (both selections get their turn)
            check_call(dg, lp, sels[which], npoints, want[which])
            _, points = dg.labels()
            other = np.arange(npoints) >= span if which == 0 else np.arange(npoints) < span
            assert (points[other] == -1).all() and not (other[ids]).any()
    dg.close()


def test_switching_graph_families_on_one_handle():
    """A shuffled path of 3000 data sets straight after a dense one-component call (the handle then expects 2
    rounds: the path needs several batches of rounds), a dense call straight after the path (the handle then
    launches 16 rounds at once).  How many rounds the path takes is the hardware's business; that it takes
    more than the first batch -- 5 rounds on a fresh handle, 3 after the dense call -- is what makes this a test
    of the batches, so it is asserted."""
    rng = np.random.RandomState(11)
    n = 3000
    path = shuffled_path(rng, n)
    dense = rng.randint(0, 40, size=(2, n)).astype(np.int64)
    fresh = _groups(path)
    check_call(fresh, path, None, n + 1)
    fresh_rounds = fresh.mean_rounds()                       # (check_call: two components calls, the same work)
    print("shuffled path of %d data sets on a fresh handle: %.1f rounds per call" % (n, fresh_rounds))
    assert fresh_rounds > 5
    fresh.close()

    dg = _groups(dense)
    calls = 0
    for lp, npoints in ((dense, 40), (path, n + 1), (dense, 40), (path, n + 1), (path, n + 1), (dense, 40)):
        set_ids(dg, lp)
        before = dg.mean_rounds() * calls
        ncomp, ids = dg.components(None, npoints)
        calls += 1
        rounds = dg.mean_rounds() * calls - before
        assert ncomp == 1 and np.array_equal(ids, np.unique(lp))
        if lp is path:
            assert rounds > 3.5
        check_call(dg, lp, None, npoints)
        calls += 2
        # cut in two
        keep = np.flatnonzero(~(lp == 20).any(axis=0))
        check_call(dg, lp, keep, npoints)
        calls += 2
    dg.close()


def test_set_ids_twice_follows_the_second_matrix():
    rng = np.random.RandomState(21)
    nlive, ndata = 10, 90
    first = clustered_ids(rng, nlive, ndata, 2, 50)
    second = clustered_ids(rng, nlive, ndata, 5, 31)[:, ::-1].copy()
    dg = _groups(first)
    ncomp, ids = dg.components(None, 200)
    assert ncomp == len(cpu_groups(first, np.arange(ndata)))
    set_ids(dg, second)
    with pytest.raises(_lib.MdnsError):                       # refused, not the first matrix's labels
        dg.labels()
    with pytest.raises(_lib.MdnsError):
        dg.labels_of_ids(len(ids))
    check_call(dg, second, None, 200)
    check_call(dg, second, _subset(ndata), 200)
    same(dg.groups(None, 200), cpu_groups(second, np.arange(ndata)))
    dg.close()


def test_labels_protocol():
    """mdns_groups_id_labels replaces the list of the last call by its labels in place: once per call, not
    after the point labels took the same scratch, only with the count that call listed; nothing after the ids
    changed."""
    rng = np.random.RandomState(22)
    nlive, ndata, npoints = 9, 70, 260
    lp = clustered_ids(rng, nlive, ndata, 4, 60)
    want = cpu_groups(lp, np.arange(ndata))
    points_want = cpu_point_labels(lp, None, npoints, want)
    dg = _groups(lp)

    ncomp, ids = dg.components(None, npoints)
    _, of_ids = dg.labels_of_ids(len(ids))
    assert np.array_equal(of_ids, points_want[ids])
    with pytest.raises(_lib.MdnsError):
        dg.labels_of_ids(len(ids))                            # twice

    ncomp, ids = dg.components(None, npoints)
    labels_a, points_a = dg.labels()
    with pytest.raises(_lib.MdnsError):
        dg.labels_of_ids(len(ids))                            # the point labels overwrote the list
    labels_b, points_b = dg.labels()                          # twice: identical
    assert np.array_equal(labels_a, labels_b) and np.array_equal(points_a, points_b)
    assert np.array_equal(points_a, points_want)

    ncomp, ids = dg.components(None, npoints)
    for wrong in (len(ids) - 1, len(ids) + 1, 0):
        with pytest.raises(_lib.MdnsError):
            dg.labels_of_ids(wrong)
    _, of_ids = dg.labels_of_ids(len(ids))                    # the right count still works
    assert np.array_equal(of_ids, points_want[ids])

    ncomp, ids = dg.components(None, npoints)
    dg.replace([3], [2], [5])
    with pytest.raises(_lib.MdnsError):
        dg.labels()
    with pytest.raises(_lib.MdnsError):
        dg.labels_of_ids(len(ids))
    lp[2, 3] = 5
    check_call(dg, lp, None, npoints)
    dg.close()


# ---------------------------------------------------------------------------------- D. refusals

def _refused(dg):
    """The label calls give an error return, with a message."""
    for call in (dg.labels, lambda: dg.labels_of_ids(1)):
        with pytest.raises(_lib.MdnsError) as e:
            call()
        assert "no components computed" in str(e.value)


@pytest.mark.parametrize("regrow", [False, True])
@pytest.mark.parametrize("bad", ["row", "slot"])
def test_bad_replacement_is_reported_by_the_next_call(bad, regrow):
    """A replacement that names a data set or a slot that does not exist among valid entries: the call returns
    0, the valid entries are applied, the NEXT components call fails with the replacement's message -- also
    when that call has to grow the per-id block first, which carries the bit over --, the one after succeeds."""
    rng = np.random.RandomState(31 + regrow)
    nlive, ndata = 6, 50
    lp = clustered_ids(rng, nlive, ndata, 3, 40)
    npoints = 130
    dg = _groups(lp)
    check_call(dg, lp, None, npoints)
    rows = np.array([0, 7, 20, ndata - 1])
    slots = np.array([0, 3, nlive - 1, nlive - 1])
    new = np.array([121, 122, 123, 124])
    valid = np.ones(4, dtype=bool)
    if bad == "row":
        rows[1], valid[1] = ndata, False
    else:
        slots[2], valid[2] = nlive, False
    lp[slots[valid], rows[valid]] = new[valid]
    dg.replace(rows, slots, new)                              # returns 0: nothing waits for the device
    ask = 5000 if regrow else npoints                         # beyond the 4096 ids the block starts with
    with pytest.raises(_lib.MdnsError) as e:
        dg.components(None, ask)
    assert "earlier mdns_groups_replace" in str(e.value)
    _refused(dg)
    assert np.array_equal(dg.ids(), lp)
    check_call(dg, lp, None, ask)
    same(dg.groups(None, ask), cpu_groups(lp, np.arange(ndata)))
    check_call(dg, lp, _subset(ndata), npoints)
    dg.close()


def test_a_failed_call_leaves_no_labels():
    """After a good call, one that fails -- an id beyond npoints, no room for the list -- has already replaced
    labels and stamps: mdns_groups_labels / _id_labels are refused instead of returning them as the last
    call's."""
    rng = np.random.RandomState(41)
    nlive, ndata = 7, 60
    lp = clustered_ids(rng, nlive, ndata, 3, 45)
    npoints = int(lp.max()) + 1
    dg = _groups(lp)
    check_call(dg, lp, None, npoints)
    ncomp, ids = dg.components(None, npoints)

    with pytest.raises(_lib.MdnsError) as e:
        dg.components(None, npoints - 1)                      # the highest id is out of range
    assert "outside" in str(e.value)
    _refused(dg)
    check_call(dg, lp, None, npoints)

    ncomp, ids = dg.components(None, npoints)
    rc, _, nd, _, _ = raw_components(dg, np.arange(ndata - 1), npoints, cap=len(ids) // 2)
    assert rc != 0 and "room for" in _lib.last_error()
    _refused(dg)
    rc, ncomp2, nd, distinct, _ = raw_components(dg, None, npoints, cap=len(ids))
    assert rc == 0 and ncomp2 == ncomp and nd == len(ids) and np.array_equal(distinct[:nd], ids)
    check_call(dg, lp, _subset(ndata), npoints)
    dg.close()


def test_arguments_are_checked_and_the_handle_survives():
    lib = _lib.require_device()
    for nlive, ndata in ((0, 5), (5, 0), (0, 0), (-1, 3)):
        assert not lib.mdns_groups_create(nlive, ndata)
        assert _lib.last_error()
    lp = np.arange(40, dtype=np.int64).reshape(4, 10)        # ten data sets that share nothing
    ids32 = np.ascontiguousarray(lp, dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    # a handle without ids
    h = lib.mdns_groups_create(4, 10)
    assert h
    ncomp = C.c_int(-7)
    assert lib.mdns_groups_components(h, None, 10, 40, C.addressof(ncomp), None, None, 0, None) != 0
    assert "no id matrix" in _lib.last_error()
    assert lib.mdns_groups_replace(h, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), 1) != 0
    assert "no id matrix" in _lib.last_error()
    assert lib.mdns_groups_set_ids(h, _lib.ptr(ids32)) == 0  # usable afterwards
    assert lib.mdns_groups_components(h, None, 10, 40, C.addressof(ncomp), None, None, 0, None) == 0 and ncomp.value == 10
    lib.mdns_groups_destroy(h)

    dg = _groups(lp)
    refusals = [
        (True, lambda: raw_components(dg, None, 40, cap=40, M=0)[0]),
        (True, lambda: raw_components(dg, np.arange(3), 40, cap=40, M=0)[0]),
        (True, lambda: raw_components(dg, None, 0, cap=40)[0]),
        (True, lambda: raw_components(dg, None, 40, cap=40, M=9)[0]),       # rows == NULL needs M == ndata
        (True, lambda: raw_components(dg, None, 40, cap=40, M=11)[0]),
        (False, lambda: lib.mdns_groups_replace(dg._h, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), -1)),
        (False, lambda: lib.mdns_groups_replace(dg._h, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), 11)),
        (False, lambda: lib.mdns_groups_replace(dg._h, None, _lib.ptr(one), _lib.ptr(one), 1)),
    ]
    for is_components, call in refusals:
        check_call(dg, lp, None, 40)
        assert call() != 0
        assert _lib.last_error()
        if is_components:
            _refused(dg)                                      # any components call that fails
        assert np.array_equal(dg.ids(), lp)
        check_call(dg, lp, np.array([0, 3, 9]), 40)
    dg.close()


# ---------------------------------------------------------------------------------- E. the stamps start over

def test_stamps_start_over():
    """Call numbers stamp the point labels; at 0x7ffffff0 the stamps are cleared and the numbers restart at 1.
    The test entry point puts the counter just below: two disjoint selections alternate across the restart, a
    shuffled path that needs several batches (whose flags take numbers beyond the threshold) is the last call
    before it and takes the threshold itself as its stamp.  Six small selections are looked at once at the very
    start and never again, so their ids keep the stamps of the first dozen calls: after the restart the calls
    with those numbers must not find them."""
    rng = np.random.RandomState(51)
    n, side, small = 3000, 40, 8
    base = n + 1
    blocks = [base + rng.randint(0, 30, size=(2, side)), base + 100 + rng.randint(0, 30, size=(2, side))]
    blocks += [base + 200 + 20 * k + rng.randint(0, 20, size=(2, small)) for k in range(6)]
    lp = np.concatenate([shuffled_path(rng, n)] + blocks, axis=1).astype(np.int64)
    npoints = base + 330
    path = np.arange(n)
    A, B = n + np.arange(side), n + side + np.arange(side)
    early = [n + 2 * side + small * k + np.arange(small) for k in range(6)]
    dg = _groups(lp)
    assert debug_set_call(dg, 0) == 0
    for rows in early:                                        # calls 1 ... 12 (or a few more)
        check_call(dg, lp, rows, npoints)
    assert debug_set_call(dg, 1) != 0 and "below" in _lib.last_error()      # forward only
    assert debug_set_call(dg, STAMP_WRAP + 1) != 0            # not past the threshold
    assert debug_set_call(dg, STAMP_WRAP - 40) == 0
    check_call(dg, lp, A, npoints)
    check_call(dg, lp, B, npoints)
    calls = 2 * len(early) + 4
    assert debug_set_call(dg, STAMP_WRAP - 1) == 0
    before = dg.mean_rounds() * calls
    ncomp, ids = dg.components(path, npoints)                 # STAMP_WRAP itself, its later batches beyond
    assert ncomp == 1 and np.array_equal(ids, np.arange(n + 1))
    assert dg.mean_rounds() * (calls + 1) - before > 5.5     # more than the first batch
    labels, points = dg.labels()
    assert not labels.any() and np.array_equal(points, cpu_point_labels(lp, path, npoints))
    assert debug_set_call(dg, STAMP_WRAP - 1) != 0            # (the counter did pass the threshold)
    for k in range(8):                                        # 1, 2, ... again
        check_call(dg, lp, (A, B)[k % 2], npoints)
    assert debug_set_call(dg, 100) == 0                       # (and did start over)
    check_call(dg, lp, None, npoints)
    dg.close()


# ---------------------------------------------------------------------------------- F. the core's device branch

@pytest.mark.parametrize("seed", range(6))
def test_core_groups_from_the_device(seed):
    """tests/test_core.py's planted matrices with a device grouping behind the core and no selection small
    enough for the host's union-find: groups_graph assembles ordered groups from the device's labels (original
    data-set indices) and id labels -- fresh and focussed, the fewer-than-2-nlive-ids shortcut included --
    against scipy."""
    from massivedatans_amd import constrainer, core
    from test_core import _core, _groups as core_groups, _planted, _scipy_groups
    rng = np.random.RandomState(seed)
    ndata, nlive = [(60, 6), (200, 10), (400, 8), (150, 20), (300, 5), (500, 12)][seed]
    lp, npoints = _planted(rng, ndata, nlive, ncommunities=[3, 6, 12, 4, 20, 8][seed], bridges=[2, 6, 20, 3, 30, 10][seed])
    L, plain, _ = _core(nlive, ndata)                        # (skips without the core; declares the debug calls)
    L.mdns_core_destroy(plain)
    dg = _groups(lp)
    gb = core.device_group_backend(dg)
    be, prior = constrainer.DrawBackend(), constrainer.sample_py_prior()
    mt = np.zeros(700, dtype=np.uint32)
    h = L.mdns_core_create(nlive, ndata, 3, 10, 1, 2, 1000, 20, 1, C.addressof(be), C.addressof(prior), None,
                           mt.ctypes.data, C.addressof(gb), None, None)
    assert h
    L.mdns_core_set_host_edges(h, 0)
    ids32 = np.ascontiguousarray(lp, dtype=np.int32)
    assert L.mdns_core_debug_set_ids(h, ids32.ctypes.data, npoints, 0) == 0
    nsplit = 0
    for chain in range(4):
        # focussed passes: kept up to date on the host and compared by the library itself with a fresh grouping
        # from the device; or (no incremental analysis) every one of them straight from the device
        if chain % 2 == 0:
            L.mdns_core_set_incremental(h, 4000000, 1)
        else:
            L.mdns_core_set_incremental(h, 0, 0)
        sel = np.flatnonzero(rng.uniform(size=ndata) < rng.uniform(0.5, 1.0))
        first = True
        while len(sel) > 0:
            want = _scipy_groups(lp, sel, nlive)
            assert core_groups(L, h, sel, nlive, focussed=False, restart=False) == want
            assert core_groups(L, h, sel, nlive, focussed=True, restart=first) == want
            nsplit += len(want) > 1
            first = False
            leave = rng.uniform(size=len(sel)) < rng.choice([0.1, 0.3, 0.5])
            if not leave.any():
                leave[rng.randint(len(sel))] = True
            sel = sel[~leave]
    stats = np.zeros(len(core.COUNTERS), dtype=np.int64)
    L.mdns_core_stats(h, stats.ctypes.data)
    s = dict(zip(core.COUNTERS, stats.tolist()))
    assert s["groupings_device"] > 0 and s["groupings_host"] == 0
    assert nsplit > 0, "no selection ever fell into several groups: the test would be vacuous"
    # The reference's shortcut: fewer than 2 nlive distinct ids make ONE group whatever the graph says.  With
    # distinct ids in every column two components hold at least 2 nlive ids, so it only shows with a column
    # that repeats an id: two data sets, each holding one id of its own nlive times -- two components on the
    # device, one group from the core.
    lp2 = lp.copy()
    lp2[:, 0] = lp[0, 0]
    lp2[:, 1] = (lp[0, 0] + 3 * nlive) % npoints              # (an id of another community's pool)
    set_ids(dg, lp2)
    ids32 = np.ascontiguousarray(lp2, dtype=np.int32)
    assert L.mdns_core_debug_set_ids(h, ids32.ctypes.data, npoints, 0) == 0
    L.mdns_core_set_incremental(h, 0, 0)
    pair = np.array([0, 1])
    want = _scipy_groups(lp2, pair, nlive)
    assert len(want) == 1 and len(cpu_groups(lp2, pair)) == 2
    assert core_groups(L, h, pair, nlive, focussed=False, restart=False) == want
    assert core_groups(L, h, pair, nlive, focussed=True, restart=True) == want
    L.mdns_core_stats(h, stats.ctypes.data)
    assert dict(zip(core.COUNTERS, stats.tolist()))["groupings_device"] == s["groupings_device"] + 2
    L.mdns_core_destroy(h)
    dg.close()
