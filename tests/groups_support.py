"""Test helpers of the grouping kernels' shape suite (test_groups_shapes.py, groups_cases.py): the derived CPU
statements -- point labels and the bit map of the ids held, both from ``cpu_groups`` of test_groups.py (scipy's
connected components + numpy.unique) --, vectorised generators of id matrices, and ``check_call``, which compares
everything one selection on one handle has to give.  Integer results throughout: every comparison is exact."""
import ctypes as C

import numpy as np

from massivedatans_amd import _lib
from test_groups import clustered_ids, cpu_groups

#: where mdns_groups_components starts the stamps over (csrc/mdns_groups.hip)
STAMP_WRAP = 0x7ffffff0
#: threads of k_groups_compact: a thread lists ``ceil(nwords / COMPACT_THREADS)`` words of the bit map
COMPACT_THREADS = 1024


# ----------------------------------------------------------------------------------------------- statements

def _selection(lp, rows):
    return np.arange(lp.shape[1]) if rows is None else np.asarray(rows)


def cpu_labels(want, rows):
    """int32[M]: for every selected data set (ascending ``rows``) the lowest data set of its component, from
    the output of ``cpu_groups``."""
    rows = np.asarray(rows)
    out = np.full(len(rows), -1, dtype=np.int32)
    for members, _ in want:
        out[np.searchsorted(rows, members)] = members.min()
    return out


def cpu_point_labels(lp, rows, npoints, want=None):
    """int32[npoints]: the lowest selected data set of the component that holds the id, -1 for an id no
    selected data set holds."""
    rows = _selection(lp, rows)
    want = cpu_groups(lp, rows) if want is None else want
    out = np.full(int(npoints), -1, dtype=np.int32)
    for members, ids in want:
        out[ids] = members.min()
    return out


def cpu_touched(lp, rows, npoints):
    """uint64[ceil(npoints / 64)]: bit q of word q // 64 = some selected data set holds id q; every bit at or
    above ``npoints`` zero."""
    rows = _selection(lp, rows)
    nwords = (int(npoints) + 63) // 64
    bits = np.zeros(nwords * 64, dtype=np.uint8)
    bits[np.unique(lp[:, rows])] = 1
    assert not bits[int(npoints):].any()
    return np.packbits(bits, bitorder="little").view(np.uint64)


# ----------------------------------------------------------------------------------------------- the comparison

def set_ids(dg, lp):
    """A whole new id matrix on the handle of ``dg`` (same shape)."""
    ids = np.ascontiguousarray(lp, dtype=np.int32)
    assert ids.shape == (dg.nlive, dg.ndata)
    _lib.check(dg._lib.mdns_groups_set_ids(dg._h, _lib.ptr(ids)), "mdns_groups_set_ids")


def check_call(dg, lp, rows, npoints, want=None):
    """Everything one selection has to give, against the CPU statements: component count, ascending list and
    its length, the bit map word for word (a call of its own, through ``rows`` + ``touched`` of the C ABI),
    both arrays of ``labels()``, and ``labels_of_ids`` = the point labels of the listed ids.  Returns the
    number of components."""
    sel = _selection(lp, rows)
    want = cpu_groups(lp, sel) if want is None else want
    ids_want = np.unique(lp[:, sel])
    labels_want = cpu_labels(want, sel)
    points_want = cpu_point_labels(lp, sel, npoints, want)

    ncomp, ids = dg.components(rows, npoints)
    assert ncomp == len(want)
    assert len(ids) == len(ids_want)                         # ndistinct
    assert np.array_equal(ids, ids_want)
    labels_a, of_ids = dg.labels_of_ids(len(ids))
    assert np.array_equal(labels_a, labels_want)
    assert np.array_equal(of_ids, points_want[ids_want])

    bits = dg.touched(npoints, rows)
    bits_want = cpu_touched(lp, sel, npoints)
    assert bits.shape == bits_want.shape and np.array_equal(bits, bits_want)
    tail = int(npoints) % 64
    if tail:
        assert int(bits[-1]) >> tail == 0
    labels_b, points = dg.labels()
    assert np.array_equal(labels_b, labels_want)
    assert np.array_equal(points, points_want)
    # (the second pair of a call: the same again)
    labels_c, points_c = dg.labels()
    assert np.array_equal(labels_c, labels_b) and np.array_equal(points_c, points)
    return ncomp


def raw_components(dg, rows, npoints, cap=None, M=None, want_touched=False):
    """mdns_groups_components through ctypes with every argument the caller's: returns (return code, number of
    components, ndistinct, list buffer, bit map or None)."""
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
    if M is None:
        M = dg.ndata if rows is None else len(rows)
    room = max(int(cap) if cap is not None else 0, 1)
    distinct = np.full(room, -7, dtype=np.int32)
    bits = np.zeros((max(int(npoints), 1) + 63) // 64, dtype=np.uint64) if want_touched else None
    ncomp, nd = C.c_int(-7), C.c_longlong(-7)
    rc = dg._lib.mdns_groups_components(dg._h, None if rows is None else _lib.ptr(rows), int(M), int(npoints),
                                        C.addressof(ncomp), C.addressof(nd), None if cap is None else _lib.ptr(distinct),
                                        0 if cap is None else int(cap), None if bits is None else _lib.ptr(bits))
    return rc, int(ncomp.value), int(nd.value), distinct, bits


def debug_set_call(dg, call):
    """The test entry point of csrc/mdns_groups.hip: moves the handle's call counter forward (never back)."""
    fn = dg._lib.mdns_groups_debug_set_call
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    return fn(dg._h, int(call))


# ----------------------------------------------------------------------------------------------- generators

def compact_run(npoints):
    """Words of the bit map one thread of k_groups_compact lists."""
    nwords = (int(npoints) + 63) // 64
    return (nwords + COMPACT_THREADS - 1) // COMPACT_THREADS


def fill_columns(ids, nlive, ndata):
    """int64[nlive, ndata] that holds the given ids (all of them when there are at most nlive * ndata), data set
    d the stretch ids[d * nlive ...] of the list repeated cyclically: distinct within a column whenever the
    list has at least nlive entries."""
    ids = np.asarray(ids, dtype=np.int64)
    flat = ids[np.arange(nlive * ndata) % len(ids)]
    return np.ascontiguousarray(flat.reshape(ndata, nlive).T)


def sparse_edge_ids(npoints):
    """The ids at which the one-workgroup compaction hands over: bits 0 and 63 of the last word of thread
    k - 1 and the first of thread k, for k at the scan's wave boundaries (63, 64, 65), in the middle (512) and
    at the last thread (1023), plus id 0 and the last id."""
    run = compact_run(npoints)
    ids = {0, int(npoints) - 1}
    for k in (1, 63, 64, 65, 512, 1023):
        for word in (k * run - 1, k * run):
            for bit in (0, 63):
                q = word * 64 + bit
                if 0 <= q < npoints:
                    ids.add(q)
    return np.array(sorted(ids), dtype=np.int64)


def dense_matrix(npoints, nlive, ndata):
    """Every id of [0, npoints) held: data set d holds the stretch [d * nlive, (d + 1) * nlive) modulo npoints."""
    assert nlive * ndata >= npoints
    return fill_columns(np.arange(npoints), nlive, ndata)


def random_matrix(rng, npoints, nlive, ndata, fraction=0.3):
    """About ``fraction`` of the ids held (at most nlive * ndata), drawn by one permutation."""
    n = max(1, min(int(round(fraction * npoints)), nlive * ndata))
    return fill_columns(rng.permutation(int(npoints))[:n], nlive, ndata)


def family_matrix(rng, family, nlive, M):
    """(int64[nlive, M], npoints) of one graph family over M data sets; ids of a column distinct.
    disjoint: M components.  bridge: two columns share the id in their LAST slot (the slot of the final,
    partial lane trip of a wave).  path: column j's last id is column j + 1's first, columns shuffled (one id
    for all when nlive is 1: a column has nothing else to share).  clustered: test_groups.clustered_ids."""
    own = np.arange(nlive * M, dtype=np.int64).reshape(M, nlive).T        # column j: [j * nlive, (j + 1) * nlive)
    npoints = nlive * M + 5
    if family == "disjoint":
        lp = own.copy()
    elif family == "bridge":
        lp = own.copy()
        if M > 1:
            lp[nlive - 1, M - 1] = lp[nlive - 1, M // 3]
    elif family == "path":
        if nlive == 1:
            lp = np.zeros((1, M), dtype=np.int64)
        else:
            lp = own.copy()
            lp[0, 1:] = own[nlive - 1, :-1]
            lp = lp[:, rng.permutation(M)]
    elif family == "clustered":
        pool = 2 * nlive + 3
        lp = clustered_ids(rng, nlive, M, 3, pool)
        npoints = 3 * pool + 5
    else:
        raise ValueError(family)
    # slots in random order: what sits in a wave's last lane trip differs from column to column
    if family != "bridge":
        lp = np.take_along_axis(lp, np.argsort(rng.uniform(size=lp.shape), axis=0), axis=0)
    return np.ascontiguousarray(lp), npoints


def embed(rng, lp, npoints, columns, ndata):
    """The matrix ``lp`` placed in the given columns of a larger one; every other column holds ids drawn from
    the whole range, so that it would join components and add ids if it were read."""
    nlive = lp.shape[0]
    big = rng.randint(0, npoints, size=(nlive, ndata)).astype(np.int64)
    big[:, columns] = lp
    return big


def shuffled_path(rng, n):
    """Data set d holds ids d and d + 1, the data sets in random order: one component of diameter n."""
    return np.vstack([np.arange(n), np.arange(n) + 1])[:, rng.permutation(n)]
