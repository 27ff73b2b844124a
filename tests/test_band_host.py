"""The statement, the edge solver and the case generators of tests/band_support.py on synthetic likelihoods: what
test_band_planted.py holds the device to is itself held to ``constrainer.python_backend``'s ``draw_band`` (the numpy
backend a CPU run uses), to the classes every case must contain, and to the ``(npairs, cap)`` table of
``mdns_backend_draw_band_end``.  No device."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import constrainer, jointstate
import band_support as bs

SHAPES = ((2, 64), (3, 130), (9, 200), (33, 70))


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def case(request):
    B, M = request.param
    L = bs.synthetic_L(B, M, 100 * B + M)
    assert (L < 0).all() and np.abs(L).min() >= 1e1 and np.abs(L).max() <= 1e7 * (B + 1.5)
    edge, misses = bs.edge_rounds(L)
    return {"L": L, "edge": edge, "misses": misses, "graded": bs.graded_rounds(L)}


def test_the_solver_finds_every_edge(case):
    """No miss among the edges the case asks for, and each solution is what it is said to be: on the edge exactly, its
    one-ulp neighbour on the other side; and none among 3000 random values at |v| ~ 1e2, 3e5 and 1e7."""
    assert case["misses"] == []
    rng = np.random.RandomState(7)
    for mag in (1e2, 3e5, 1e7):
        for v in -mag * rng.uniform(0.5, 2.0, size=1000):
            upper, lower = bs.edge_thresholds(v)
            assert upper is not None and lower is not None, v
            assert upper + 1e-12 * (abs(v) + abs(upper)) == v and upper < v
            assert lower - 1e-12 * (abs(v) + abs(lower)) == v and lower > v
            below, above = np.nextafter(upper, -np.inf), np.nextafter(lower, np.inf)
            assert v > below + 1e-12 * (abs(v) + abs(below))
            assert not v >= above - 1e-12 * (abs(v) + abs(above))


def test_every_class_occurs_in_every_case(case):
    L = case["L"]
    seen = bs.seen_classes(L, case["edge"])
    assert seen >= set(bs.REQUIRED) | set(bs.EDGE_KINDS), (set(bs.REQUIRED) | set(bs.EDGE_KINDS)) - seen
    seen = bs.seen_classes(L, case["graded"])
    want = set(bs.GRADED_KINDS) | {"status0", "status1", "status2", "clear-with-pairs"}
    assert seen >= want, want - seen
    bounds = np.concatenate([rd["bound"] for rd in case["graded"]])
    assert set(bounds) == set(bs.BOUNDS)
    for rd in case["graded"]:
        assert (rd["bound"] == 0.0).any() or len(rd["bound"]) < 3


def test_no_graded_pair_is_ambiguous(case):
    for rd in case["graded"]:
        assert int(bs.ambiguous(case["L"], rd["thr"], rd["bound"]).sum()) == 0, rd["name"]
    # (the rule bites: a likelihood exactly on the upper edge of a band with a bound is ambiguous, without a bound it is not)
    v = 1.01
    for _ in range(4):
        v = 1.01 * 1.0 + 1e-12 * (abs(v) + 0.0)
    L, thr = np.array([[v]]), np.array([0.0])
    assert bs.band_of(L, thr, np.array([1.0]))[0, 0] == v
    assert bs.ambiguous(L, thr, np.array([1.0]))[0, 0]
    upper = bs.edge_thresholds(-3e5)[0]
    assert not bs.ambiguous(np.array([[-3e5]]), np.array([upper]), np.array([0.0]))[0, 0]


class PlantedScorer(object):
    """answers the planted block: candidate ``params[:, 0]`` (its number), the data sets of ``mask``"""

    def __init__(self, L):
        self.L = L

    def loglike_batch(self, params, mask):
        return self.L[np.asarray(params)[:, 0].astype(int)][:, mask]


def _scored_prefix(L, thr, bound):
    """how many candidates ``python_backend``'s draw_band scores: pieces of 1, 2, 4 ... up to the piece that holds a
    candidate some data set accepts whatever the noise (nobody looks behind it: those count as -inf)"""
    clear = bs.classes(L, thr, bound)[0].any(axis=1)
    pos, piece = 0, 1
    while pos < len(L):
        end = min(len(L), pos + piece)
        if clear[pos:end].any():
            return end
        pos, piece = end, min(64, 2 * piece)
    return len(L)


def _backend_band(be, B, bound, cap):
    p = np.ascontiguousarray(np.arange(B, dtype=np.float64).reshape(B, 1))
    status, npairs = np.full(B, -7, dtype=np.int32), C.c_int(-1)
    pb, pk, pL, pthr = np.full(cap, -7, dtype=np.int32), np.full(cap, -7, dtype=np.int32), np.full(cap, -7.0), np.full(cap, -7.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = be.draw_band(None, p.ctypes.data_as(dp), B, np.ascontiguousarray(bound).ctypes.data_as(dp), status.ctypes.data_as(ip), C.byref(npairs),
                      pb.ctypes.data_as(ip), pk.ctypes.data_as(ip), pL.ctypes.data_as(dp), pthr.ctypes.data_as(dp), cap)
    assert rc == 0
    return status, npairs.value, pb, pk, pL, pthr


@pytest.mark.parametrize("selection", ("all", "sparse"))
def test_the_statement_is_the_python_backends(case, selection):
    """Status, pair set and ``npairs`` (against a large and a small ``cap``) of ``python_backend``'s ``draw_band`` over a
    ``HostJointState`` whose scorer returns the planted block."""
    L = case["L"]
    B, M = L.shape
    rows = None if selection == "all" else np.sort(np.random.RandomState(M).choice(M, size=M // 2, replace=False)).astype(np.int32)
    sel = np.arange(M) if rows is None else rows
    host = jointstate.HostJointState(PlantedScorer(L), 6, M, lambda p: p, nparams=1)
    be = constrainer.python_backend(host)
    dp_int = C.POINTER(C.c_int)
    for rd in case["edge"] + case["graded"]:
        host.live = bs.live_for(rd["thr"], 6)
        host.shelfL = [[] for _ in range(M)]
        host.set_running(np.arange(M))
        host.prepare()
        assert np.array_equal(host.higher, rd["thr"])
        n = _scored_prefix(L[:, sel], rd["thr"][sel], rd["bound"])
        Leff = np.vstack((L[:n, sel], np.full((B - n, len(sel)), -np.inf)))
        want = bs.statement(Leff, rd["thr"][sel], rd["bound"])
        for cap in (4096, 3):
            assert be.draw_begin(None, rows.ctypes.data_as(dp_int) if rows is not None else None, len(sel)) == 0
            with np.errstate(invalid="ignore"):             # (inf - inf at the thresholds +-inf)
                status, npairs, pb, pk, pL, pthr = _backend_band(be, B, rd["bound"], cap)
            assert np.array_equal(status, want["status"]), rd["name"]
            assert npairs == want["npairs"], rd["name"]
            m = min(npairs, cap)
            assert np.array_equal(pb[:m], want["pair_b"][:m]) and np.array_equal(pk[:m], want["pair_k"][:m])
            assert np.array_equal(pL[:m], want["pair_L"][:m]) and np.array_equal(pthr[:m], want["pair_thr"][:m])
            assert (pb[m:] == -7).all() and (pL[m:] == -7.0).all()


@pytest.mark.parametrize("cap", (1, 64, 4096, 5000))
def test_the_table_of_end(cap):
    """``room = min(cap, 4096)`` entries at most leave the device's box -- never more than it holds, never more than the
    caller has room for; ``*npairs`` is the true count where everything was handed over and above ``cap`` otherwise."""
    for n in (0, cap - 1, cap, cap + 1, 4095, 4096, 4097, 6000):
        copied, npairs = bs.end_table(n, cap)
        assert 0 <= copied <= min(cap, 4096, n)
        if n <= min(cap, 4096):
            assert (copied, npairs) == (n, n)
        else:
            assert copied == min(cap, 4096) and npairs > cap
            assert npairs == (n if n > cap else cap + 1)
        assert (npairs <= cap) == (copied == n == npairs), "the caller takes the list exactly when it is whole"
