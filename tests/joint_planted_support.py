"""Planted joint states (test_joint_planted.py on the device, test_joint_planted_host.py on the numpy statement).

A fixed-scale state (``like.WeightedSpectra``) over spectra with ``y = 0``, ``v = 1``, scored with all-zero curves,
gives ``L = -0`` for every (candidate, data set) pair, and the ``jitter[B, M]`` block of a chunk is added to that: the
likelihood of every pair is the planted double, bit for bit, +-inf and NaN included.  So a chunk tests
``k_joint_accept_dense`` / ``k_joint_commit_dense`` on exact values, and a sequence of single-candidate chunks plants any
shelf; the live matrix is then overwritten in place and ``prepare`` computes everything from the two arrays alone.

Here: the brute-force reference :class:`Reference` (numpy, not ``HostJointState``), one driver per kind of state with
the same few methods, the planting sequence, the comparisons and the case generators.  NaN occurs among candidates
only: what a NaN among the live points means is not defined."""
import numpy as np

NX = 8
#: the live value of the planting phase: every threshold is this, so any finite or +inf value is accepted
LOW = -1e300
HELD = 128        # shelf entries / live slots a data set's sixteen lanes hold in registers (k_joint_prepare)

DROP_PATTERNS = ("none", "all", "head", "tail", "alternate", "batch16", "first128", "beyond128", "equal")
TIE_PAIRS = ((0, 16), (1, 16), (5, 130), (127, 128))
THRESHOLD_KINDS = ("multiple", "live", "shelf", "far-live", "far-shelf", "inf")
COMMIT_KINDS = ("same", "below", "equal", "above", "inf-accepted", "became-inf", "inf-refused", "on-threshold", "one-ulp", "nan")
#: running-list lengths the read-out of ``case_readout`` must pass through
NRUN_SCHEDULE = (65, 64, 63, 17, 16, 15, 5, 4, 3, 2, 1)


# ---------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------
class Reference(object):
    """Per data set: ``Lmin = live.min()``, ``argmin`` its first occurrence, ``keep = shelf > Lmin``, ``kept =
    shelf[keep]`` in order, ``higher = sort(concat(live, kept))[len(kept)]``.  A commit appends L where ``L > higher``
    and recomputes ``higher`` the same way; an advance puts ``kept[0]`` into slot ``argmin`` and shifts the rest."""

    def __init__(self, nlive, ndata):
        self.nlive, self.ndata = nlive, ndata
        self.live = np.full((nlive, ndata), LOW)
        self.shelf = [np.zeros(0) for _ in range(ndata)]
        self.higher = np.full(ndata, np.nan)
        self.argmin = np.zeros(ndata, dtype=int)
        self.running = np.arange(ndata)
        self.seen = set()                                  # COMMIT_KINDS that occurred

    def _threshold(self, d):
        kept = self.shelf[d]
        return np.sort(np.concatenate((self.live[:, d], kept)))[len(kept)]

    def sizes(self):
        return np.array([len(s) for s in self.shelf])

    def prepare(self):
        """-> Lmin [nrun], argmin [nrun], keep (one bool array per running data set, as long as its shelf was)"""
        Lmin, arg, keeps = [], [], []
        for d in self.running:
            col = self.live[:, d]
            m = col.min()
            a = int(np.flatnonzero(col == m)[0])
            keep = self.shelf[d] > m
            self.shelf[d] = self.shelf[d][keep]
            self.higher[d] = self._threshold(d)
            self.argmin[d] = a
            Lmin.append(m)
            arg.append(a)
            keeps.append(keep)
        return np.array(Lmin), np.array(arg, dtype=int), keeps

    def chunk(self, L, rows):
        """L [B, M] over ``rows`` (None: all) -> (accepted index or -1, who it beats [M] or None)"""
        rows = np.arange(self.ndata) if rows is None else np.asarray(rows)
        thr = self.higher[rows]
        with np.errstate(invalid="ignore"):
            ok = L > thr
        if (L == np.inf)[:, thr == np.inf].any():
            self.seen.add("inf-refused")
        if not ok.any():
            return -1, None
        idx = int(np.argmax(ok.any(axis=1)))
        beats = ok[idx]
        if (L[:idx + 1] == thr).any():
            self.seen.add("on-threshold")
        if np.isnan(L[:idx + 1]).any():
            self.seen.add("nan")
        for d, v in zip(rows[beats], L[idx][beats]):
            old = self.higher[d]
            values = np.concatenate((self.live[:, d], self.shelf[d]))
            above = values[values > old]
            nxt = above.min() if len(above) else np.inf
            self.shelf[d] = np.append(self.shelf[d], v)
            new = self.higher[d] = self._threshold(d)
            if v == np.nextafter(old, np.inf):
                self.seen.add("one-ulp")
            if v == np.inf:
                self.seen.add("inf-accepted")
            if new == old:
                self.seen.add("same")
            elif new == np.inf:
                self.seen.add("became-inf")
            if new != old and nxt < np.inf:
                self.seen.add("below" if v < nxt else "equal" if v == nxt else "above")
        return idx, beats

    def advance(self):
        for d in self.running:
            self.live[self.argmin[d], d] = self.shelf[d][0]
            self.shelf[d] = self.shelf[d][1:]


def pack_bits(bits):
    """bool [n] -> uint64 [ceil(n / 64)], bit k of word k / 64 = bits[k], the rest zero"""
    bits = np.asarray(bits, dtype=bool)
    padded = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


def keep_words(keeps, kw):
    """The keep words ``mdns_joint_prepare`` must give for the reference's ``keeps``: uint64 [nrun, kw]; bits at and
    beyond a shelf's length, and whole words beyond it, are zero."""
    out = np.zeros((len(keeps), kw), dtype=np.uint64)
    for r, k in enumerate(keeps):
        w = pack_bits(k)
        assert len(w) <= kw
        out[r, :len(w)] = w
    return out


# ---------------------------------------------------------------------------------------
# the two kinds of state behind one set of methods
# ---------------------------------------------------------------------------------------
class DeviceDriver(object):
    """``CurveJointState`` over zero spectra with unit variances at fixed scale, scored with zero curves."""

    def __init__(self, nlive, ndata, shelf_cap=4):
        from massivedatans_amd import _lib, jointstate
        from massivedatans_amd.like import WeightedSpectra
        self._lib_module = _lib
        self.nlive, self.ndata = nlive, ndata
        self.spectra = WeightedSpectra(np.linspace(1.0, 2.0, NX), np.zeros((NX, ndata)), np.ones((NX, ndata)))
        self.js = jointstate.CurveJointState(self.spectra, nlive, lambda xs: np.zeros((len(xs), NX)), shelf_cap=shelf_cap, ndim=1)
        self.lib, self.h = self.js._lib, self.js._h

    def close(self):
        self.js.close()
        self.spectra.close()

    def _check(self, rc, what):
        self._lib_module.check(rc, what)

    def set_live(self, live):
        """(empties the shelves)"""
        live = np.ascontiguousarray(live, dtype=np.float64)
        assert live.shape == (self.nlive, self.ndata)
        self._check(self.lib.mdns_joint_set_live(self.h, self._lib_module.ptr(live)), "mdns_joint_set_live")

    def overwrite_live(self, live):
        """the live matrix in place: shelves and thresholds stay as they are"""
        live = np.ascontiguousarray(live, dtype=np.float64)
        assert live.shape == (self.nlive, self.ndata)
        self._check(self.lib.mdns_h2d(self.lib.mdns_joint_live_dev(self.h), self._lib_module.ptr(live), live.nbytes), "mdns_h2d")

    def set_running(self, running):
        self.js.set_running(running)

    def keep_width(self):
        return self.lib.mdns_joint_keep_words(self.h)

    def shelf_cap(self):
        return self.lib.mdns_joint_shelf_cap(self.h)

    def prepare(self):
        """-> Lmin, argmin, the raw keep words uint64 [nrun, keep_width()]"""
        n, kw = len(self.js.running), self.keep_width()
        Lmin, arg = np.empty(n), np.empty(n, dtype=np.int32)
        words = np.full((n, kw), np.uint64(0xdeadbeefdeadbeef), dtype=np.uint64)
        ptr = self._lib_module.ptr
        self._check(self.lib.mdns_joint_prepare(self.h, ptr(Lmin), ptr(arg), ptr(words)), "mdns_joint_prepare")
        return Lmin, arg.astype(int), words

    def chunk(self, L, rows):
        """L [B, M] -> (accepted index or -1, the raw fill words uint64 [ceil(M / 64)] or None)"""
        B, M = L.shape
        idx, _, beats, n = self.js.draw_params(np.zeros((B, 1)), rows, jitter=L)
        assert n == B
        if idx < 0:
            return -1, None
        words = self.js._bits[:(M + 63) // 64].copy()
        assert np.array_equal(pack_bits(beats), words)
        return idx, words

    def advance(self):
        self.js.advance()

    def undo_advance(self):
        self._check(self.lib.mdns_joint_undo_advance_dev(self.h), "mdns_joint_undo_advance_dev")

    def live_matrix(self):
        full = np.empty((self.nlive, self.ndata))
        self._check(self.lib.mdns_joint_get_live(self.h, self._lib_module.ptr(full)), "mdns_joint_get_live")
        return full

    def thresholds(self):
        return self.js.thresholds()


class ZeroScorer(object):
    def loglike_batch(self, params, mask):
        return np.full((len(params), int(np.sum(mask))), -0.0)


class HostDriver(object):
    """``HostJointState`` over a scorer that answers -0 for every pair."""

    def __init__(self, nlive, ndata, shelf_cap=4):
        from massivedatans_amd import jointstate
        self.nlive, self.ndata = nlive, ndata
        self.js = jointstate.HostJointState(ZeroScorer(), nlive, ndata, lambda xs: xs, nparams=1)

    def close(self):
        pass

    def set_live(self, live):
        self.js.live = np.array(live, dtype=np.float64)
        self.js.shelfL = [[] for _ in range(self.ndata)]

    def overwrite_live(self, live):
        self.js.live = np.array(live, dtype=np.float64)

    def set_running(self, running):
        self.js.set_running(running)

    def keep_width(self):
        return max(1, (max(len(s) for s in self.js.shelfL) + 63) // 64)

    def shelf_cap(self):
        return None

    def prepare(self):
        run = self.js.running
        lengths = np.array([len(self.js.shelfL[d]) for d in run])
        kw = self.keep_width()
        Lmin, arg, keep = self.js.prepare()
        after = np.array([len(self.js.shelfL[d]) for d in run])
        assert (keep is None) == bool((after == lengths).all()), "keep is None exactly when nothing was dropped"
        if keep is None:
            keep = np.arange(max(lengths.max(), 1))[None, :] < lengths[:, None]
        assert not (keep & (np.arange(keep.shape[1])[None, :] >= lengths[:, None])).any()
        return Lmin, np.asarray(arg, dtype=int), keep_words([k[:n] for k, n in zip(keep, lengths)], kw)

    def chunk(self, L, rows):
        idx, Lrow, beats, n = self.js.draw_params(np.zeros((len(L), 1)), rows, jitter=L)
        if idx < 0:
            return -1, None
        return idx, pack_bits(beats)

    def advance(self):
        self.js.advance()

    def live_matrix(self):
        return self.js.live.copy()

    def thresholds(self):
        return self.js.thresholds()


# ---------------------------------------------------------------------------------------
# planting and comparing
# ---------------------------------------------------------------------------------------
def same_state(driver, ref, what):
    higher, n = driver.thresholds()
    assert np.array_equal(n, ref.sizes()), (what, "shelf sizes")
    assert np.array_equal(higher, ref.higher), (what, "thresholds")


def compare_prepare(driver, ref, what=""):
    """One ``prepare`` on both; -> what the reference found (Lmin, argmin, keeps)"""
    Lmin, arg, keeps = ref.prepare()
    if driver is None:
        return Lmin, arg, keeps
    got = driver.prepare()
    assert np.array_equal(got[0], Lmin), (what, "Lmin")
    assert np.array_equal(got[1], arg), (what, "argmin")
    assert np.array_equal(got[2], keep_words(keeps, got[2].shape[1])), (what, "keep words")
    same_state(driver, ref, what)
    return Lmin, arg, keeps


def compare_chunk(driver, ref, L, rows, what=""):
    """One chunk on both -> the reference's (index, beats)"""
    idx, beats = ref.chunk(L, rows)
    if driver is None:
        return idx, beats
    got, words = driver.chunk(L, rows)
    assert got == idx, (what, "accepted", got, idx)
    if idx >= 0:
        assert np.array_equal(words, pack_bits(beats)), (what, "fill words")
    same_state(driver, ref, what)
    return idx, beats


def start(driver, nlive, ndata):
    """Every live value LOW, shelves empty, prepared -> the reference in that state"""
    ref = Reference(nlive, ndata)
    if driver is not None:
        driver.set_running(np.arange(ndata))
        driver.set_live(ref.live)
    Lmin, arg, keeps = compare_prepare(driver, ref, "start")
    assert (ref.higher == LOW).all() and (arg == 0).all()
    return ref


def plant(driver, ref, shelves):
    """One single-candidate chunk per shelf position k: the planted entry for the data sets whose shelf is to be longer
    than k, -inf for the rest.  Every chunk must accept candidate 0 with exactly those fill bits."""
    lengths = np.array([len(s) for s in shelves])
    for k in range(lengths.max() if len(lengths) else 0):
        longer = lengths > k
        row = np.array([s[k] if len(s) > k else -np.inf for s in shelves]).reshape(1, -1)
        idx, beats = ref.chunk(row, None)
        assert idx == 0 and np.array_equal(beats, longer), ("planting entry %d is not accepted as intended" % k)
        if driver is not None:
            got, words = driver.chunk(row, None)
            assert got == 0 and np.array_equal(words, pack_bits(longer)), ("planting chunk", k)
    assert np.array_equal(ref.sizes(), lengths)
    for d, s in enumerate(shelves):
        assert np.array_equal(ref.shelf[d], s)
    if driver is not None:
        same_state(driver, ref, "planted")


def planted_state(driver, case):
    """The case's (live, shelf) pair in place and its running list set: ``prepare`` is the next call"""
    nlive, ndata = case["live"].shape
    ref = start(driver, nlive, ndata)
    plant(driver, ref, case["shelves"])
    ref.live = case["live"].copy()
    ref.running = np.asarray(case["running"])
    if driver is not None:
        driver.overwrite_live(case["live"])
        driver.set_running(ref.running)
    return ref


def read_out(driver, ref, nruns=None):
    """advance -> live matrix -> prepare, on the data sets whose shelf is not empty, until all are: every advance moves
    one head into the live matrix, so the purged shelves come out in order.  -> steps made"""
    steps = 0
    while True:
        run = ref.running[ref.sizes()[ref.running] > 0]
        if len(run) == 0:
            return steps
        steps += 1
        ref.running = run
        ref.advance()
        if driver is not None:
            driver.set_running(run)
            driver.advance()
            assert np.array_equal(driver.live_matrix(), ref.live), ("read-out step", steps)
        compare_prepare(driver, ref, ("read-out step", steps))
        if nruns is not None:
            nruns.append(len(run))


# ---------------------------------------------------------------------------------------
# what a prepare did, by name
# ---------------------------------------------------------------------------------------
def drop_patterns(shelf, keep, Lmin):
    """names of DROP_PATTERNS that ``keep`` (of a shelf as it was before the purge) shows"""
    n, out = len(keep), set()
    if n == 0:
        return out
    if keep.all():
        out.add("none")
    if not keep.any():
        out.add("all")
    if n > 1 and not keep[0] and keep[1:].all():
        out.add("head")
    if n > 1 and keep[:-1].all() and not keep[-1]:
        out.add("tail")
    if n > 1 and np.array_equal(keep, np.arange(n) % 2 == 0):
        out.add("alternate")
    if n >= 32 and not keep[16:32].any() and keep[:16].all() and keep[32:].all():
        out.add("batch16")
    if n > HELD and not keep[:HELD].any() and keep[HELD:].any():
        out.add("first128")                                # w_held == 0 with survivors beyond the registers
    if n > HELD and keep[:HELD].any() and not keep[HELD:].any():
        out.add("beyond128")
    if (shelf[~keep] == Lmin).any():
        out.add("equal")
    return out


def threshold_kinds(col, shelf, keep, thr):
    """names of THRESHOLD_KINDS: where the threshold of (live column, shelf before the purge, keep) lies"""
    out = set()
    in_live = np.flatnonzero(col == thr)
    in_shelf = np.flatnonzero((shelf == thr) & keep)       # positions before the purge: what the registers held
    if len(in_live) + len(in_shelf) > 1:
        out.add("multiple")
    if len(in_live):
        out.add("live")
    if len(in_shelf):
        out.add("shelf")
    if len(in_shelf) == 0 and len(in_live) and in_live.min() >= HELD:
        out.add("far-live")
    if len(in_live) == 0 and len(in_shelf) and in_shelf.min() >= HELD:
        out.add("far-shelf")
    if thr == np.inf:
        out.add("inf")
    return out


def tie_pairs(col):
    at = tuple(np.flatnonzero(col == col.min()))
    return {at} if at in TIE_PAIRS else set()


def run_prepare_case(driver, case, seen):
    """Plants the case, prepares, reads the shelves out; what occurred goes into ``seen`` (sets by topic)."""
    ref = planted_state(driver, case)
    if driver is not None and driver.shelf_cap() is not None and case["cap"] is not None:
        assert driver.shelf_cap() == case["cap"], "the shelves did not grow as planned"
    before = [s.copy() for s in ref.shelf]
    higher0 = ref.higher.copy()
    Lmin, arg, keeps = compare_prepare(driver, ref, case["name"])
    idle = np.setdiff1d(np.arange(ref.ndata), ref.running)
    assert np.array_equal(ref.higher[idle], higher0[idle]) and all(np.array_equal(ref.shelf[d], before[d]) for d in idle)
    seen["nrun"].add(len(ref.running))
    for r, d in enumerate(ref.running):
        col = ref.live[:, d]
        assert arg[r] == np.argmin(col)
        seen["drops"] |= drop_patterns(before[d], keeps[r], Lmin[r])
        seen["thresholds"] |= threshold_kinds(col, before[d], keeps[r], ref.higher[d])
        seen["ties"] |= tie_pairs(col)
        if Lmin[r] == -np.inf:
            seen["columns"].add("-inf")
        if (col == np.inf).all():
            seen["columns"].add("all-inf")
        elif (col == np.inf).any():
            seen["columns"].add("some-inf")
        if (col == col[0]).all() and col[0] < np.inf and len(col) > 1:
            seen["columns"].add("equal")
        seen["lengths"].add((ref.nlive, len(before[d])))
    nruns = []
    read_out(driver, ref, nruns)
    seen["nrun"] |= set(nruns)
    return ref


def new_seen():
    return {k: set() for k in ("drops", "thresholds", "ties", "columns", "lengths", "nrun")}


# ---------------------------------------------------------------------------------------
# the cases of prepare
# ---------------------------------------------------------------------------------------
def _intended_keep(pattern, n):
    keep = np.ones(n, dtype=bool)
    if pattern == "all":
        keep[:] = False
    elif pattern == "head":
        keep[:1] = False
    elif pattern == "tail":
        keep[-1:] = False
    elif pattern == "alternate":
        keep[1::2] = False
    elif pattern == "batch16":
        keep[16:32] = False
    elif pattern == "first128":
        keep[:HELD] = False
    elif pattern == "beyond128":
        keep[1:HELD:3] = False
        keep[HELD:] = False
    elif pattern == "equal":
        keep[::3] = False
    return keep


def _applies(pattern, n):
    if pattern == "none":
        return True
    if pattern in ("head", "tail", "alternate", "equal"):
        return n >= 2
    if pattern == "batch16":
        return n >= 32
    if pattern in ("first128", "beyond128"):
        return n > HELD
    return n >= 1


def _shelf(pattern, n, Lmin, rng):
    """n integer-valued entries (ties are common) that a minimum of Lmin purges by ``pattern``"""
    keep = _intended_keep(pattern, n)
    kept = Lmin + rng.randint(1, 40, size=n)
    dropped = np.full(n, Lmin) if pattern == "equal" else Lmin - rng.randint(0, 6, size=n)
    return np.where(keep, kept, dropped).astype(np.float64)


def _column(kind, nlive, Lmin, rng):
    """a live column whose minimum is Lmin (the kinds "-inf" and "all-inf" excepted)"""
    col = (Lmin + rng.randint(1, 40, size=nlive)).astype(np.float64)
    if isinstance(kind, tuple):                            # the minimum tied at exactly these slots
        col[list(kind)] = Lmin
    elif kind == "random":
        col[rng.choice(nlive, size=min(nlive, 1 + rng.randint(3)), replace=False)] = Lmin
    elif kind == "-inf":
        col[rng.randint(nlive)] = Lmin
        col[nlive // 2] = -np.inf
    elif kind == "some-inf":
        col[rng.uniform(size=nlive) < 0.4] = np.inf
        col[rng.randint(nlive)] = Lmin
    elif kind == "equal":
        col[:] = Lmin
    elif kind == "all-inf":
        col[:] = np.inf
    return col


SHELF_LENGTHS_150 = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 149)


def case_150(gapped):
    """nlive = 150: every drop pattern crossed with every shelf length it applies to, neighbouring data sets of
    different lengths; the special live columns; and columns written out for the thresholds that random values do not
    reach.  ``gapped``: one data set in seven does not run."""
    nlive = 150
    rng = np.random.RandomState(150 + gapped)
    cols, shelves = [], []

    def add(col, shelf):
        cols.append(np.asarray(col, dtype=np.float64))
        shelves.append(np.asarray(shelf, dtype=np.float64))

    for pattern in DROP_PATTERNS:
        for n in SHELF_LENGTHS_150:
            if _applies(pattern, n) and not (n == 0 and pattern != "none"):
                Lmin = float(rng.randint(-3, 4))
                add(_column("random", nlive, Lmin, rng), _shelf(pattern, n, Lmin, rng))
    for kind in TIE_PAIRS + ("-inf", "some-inf", "equal", "all-inf"):
        for n, pattern in ((0, "none"), (17, "alternate"), (129, "equal")):
            Lmin = float(rng.randint(-3, 4))
            shelf = _shelf(pattern, n, Lmin, rng)
            if kind == "some-inf" and n:
                shelf[n // 2] = np.inf                     # a +inf waiting on the shelf
            add(_column(kind, nlive, Lmin, rng), shelf)
    huge = 1e6 + np.arange(nlive)
    # the answer in the live part only, beyond the registers: three kept entries above, the 4th smallest is slot 131
    col = huge.copy()
    col[128:] = 1 + np.arange(nlive - 128)
    add(col, [500.0, 600.0, 700.0])
    # ... in the shelf part only, beyond the registers, all 149 entries kept
    col = huge.copy()
    col[0] = 0.0
    add(col, 1.0 + np.arange(149))
    # ... the same with the first 128 entries dropped (w_held == 0): the 22nd smallest is the last entry
    col = huge.copy()
    col[0] = 200.0
    add(col, np.concatenate((200.0 - np.arange(128) % 7, 201.0 + np.arange(21))))
    # ... with every other of the first 128 dropped and the far ones in reverse order
    col = huge.copy()
    col[0] = 200.0
    add(col, np.concatenate((np.where(np.arange(128) % 2 == 0, 201.0 + np.arange(128), 200.0), 400.0 - np.arange(21))))
    # the answer +inf: two finite values, three entries waiting
    col = np.full(nlive, np.inf)
    col[3] = 0.0
    add(col, [5.0, np.inf, np.inf])
    ndata = len(cols)
    assert ndata <= 300
    running = np.arange(ndata)
    if gapped:
        running = running[running % 7 != 3]
    return {"name": "nlive150-%s" % ("gapped" if gapped else "all"), "live": np.column_stack(cols), "shelves": shelves,
            "running": running, "cap": 256}


SMALL_NLIVE = (1, 15, 16, 17, 127, 128, 129)
ASCENDING_LENGTHS = (0, 1, 17, 65, 130)


def case_small(nlive):
    """Few live points and shelves longer than ``nlive - 1``: strictly ascending entries always beat the threshold of
    the planting phase; what a minimum drops of them is a prefix -- cut in front of, inside, exactly on (the strict
    comparison) and behind the entries, and at the registers' end."""
    rng = np.random.RandomState(nlive)
    cols, shelves = [], []
    kinds = ["random"] + [p for p in TIE_PAIRS if p[1] < nlive] + (["equal", "some-inf"] if nlive > 1 else [])
    for which, cut_of in enumerate((lambda n: 0, lambda n: 1, lambda n: n, lambda n: n // 2, lambda n: min(n, HELD), lambda n: min(n, HELD + 1))):
        for n in ASCENDING_LENGTHS:
            for on_entry in (False, True):
                shelf = 10.0 + 2 * np.arange(n)
                cut = cut_of(n)
                if cut == 0 or cut > n:
                    if on_entry:
                        continue
                    Lmin = 9.0
                else:
                    Lmin = shelf[cut - 1] + (0.0 if on_entry else 1.0)
                col = Lmin + 2.0 * rng.randint(1, n + 6, size=nlive)
                kind = kinds[(which + n + on_entry) % len(kinds)]
                if isinstance(kind, tuple):
                    col[list(kind)] = Lmin
                elif kind == "equal":
                    col[:] = Lmin
                else:
                    if kind == "some-inf":
                        col[rng.uniform(size=nlive) < 0.3] = np.inf
                    col[rng.randint(nlive)] = Lmin
                cols.append(col)
                shelves.append(shelf)
    ndata = len(cols)
    running = np.arange(ndata)
    if nlive % 2 == 0:
        running = running[running % 5 != 1]
    return {"name": "nlive%d" % nlive, "live": np.column_stack(cols), "shelves": shelves, "running": running, "cap": 256}


def case_readout():
    """65 running data sets, with gaps between their indices, whose shelves -- above every live value, ascending, so
    that nothing is ever dropped -- run empty one after the other: the running list shrinks through NRUN_SCHEDULE."""
    nlive, ndata = 9, 160
    rng = np.random.RandomState(65)
    chosen = np.flatnonzero(np.arange(ndata) % 7 != 2)[::2][:65]
    assert len(chosen) == 65 and (np.diff(chosen) > 1).any()
    # lengths: how many shelves hold more than t entries = the schedule
    lengths = [1, 2] + [3] * 46 + [4, 5] + [6] * 10 + [7, 8, 9, 10, 11]
    assert len(lengths) == 65
    live = rng.randint(0, 20, size=(nlive, ndata)).astype(np.float64)
    shelves = [np.zeros(0) for _ in range(ndata)]
    for d, n in zip(chosen, rng.permutation(lengths)):
        shelves[d] = 100.0 + np.cumsum(rng.randint(1, 4, size=n))
    return {"name": "read-out", "live": live, "shelves": shelves, "running": chosen, "cap": 16}


def prepare_cases():
    return [case_150(False), case_150(True)] + [case_small(n) for n in SMALL_NLIVE] + [case_readout()]


def check_prepare_coverage(seen):
    """the non-vacuity conditions of the prepare cases, on what the REFERENCE found"""
    assert seen["drops"] >= set(DROP_PATTERNS), set(DROP_PATTERNS) - seen["drops"]
    assert seen["thresholds"] >= set(THRESHOLD_KINDS), set(THRESHOLD_KINDS) - seen["thresholds"]
    assert seen["ties"] >= set(TIE_PAIRS), set(TIE_PAIRS) - seen["ties"]
    assert seen["columns"] >= {"-inf", "some-inf", "equal", "all-inf"}, seen["columns"]
    assert seen["nrun"] >= set(NRUN_SCHEDULE), set(NRUN_SCHEDULE) - seen["nrun"]
    want = {(150, n) for n in SHELF_LENGTHS_150} | {(nl, n) for nl in SMALL_NLIVE for n in ASCENDING_LENGTHS}
    assert seen["lengths"] >= want, want - seen["lengths"]


# ---------------------------------------------------------------------------------------
# the cases of the dense accept and commit
# ---------------------------------------------------------------------------------------
DENSE_M = (1, 63, 64, 65, 255, 256, 257, 300)
#: (B, candidates made acceptable); an empty list: nobody is, the outcome is -1 and nothing changes.  The only acceptable
#: one at B - 1 and at 256; several, of which the lowest wins; candidate 0 and then the same B with nobody: stale flags.
DENSE_CHUNKS = ((1, [0]), (1, []), (2, [1]), (255, [254]), (256, [255]), (257, [256]), (1024, [1023]), (1024, [256]),
                (1024, [300, 301, 900]), (257, [0]), (257, []), (1024, [0, 5]), (1024, []), (2, [0, 1]), (2, []))


def dense_case(M, gapped):
    """nlive = 5, shelves of 0 to 3 entries among the live values, and a selection of M data sets: all of M, or M of 300
    with gaps.  Columns: tie-rich integers, all equal, one finite value among +inf."""
    nlive = 5
    ndata = 300 if gapped else M
    rng = np.random.RandomState(1000 * M + gapped)
    live = rng.randint(0, 6, size=(nlive, ndata)).astype(np.float64) * 2
    for d in range(ndata):
        if d % 5 == 1:
            live[:, d] = live[0, d]
        elif d % 5 == 3:
            live[:, d] = np.inf
            live[d % nlive, d] = 3.0
    shelves = [2.0 * rng.randint(0, 8, size=d % 4) for d in range(ndata)]
    rows = None
    if gapped:
        rows = np.sort(rng.choice(np.arange(1, ndata), size=M, replace=False)).astype(np.int32)
        assert M == 1 or (np.diff(rows) > 1).any()
    return {"name": "M%d-%s" % (M, "gapped" if gapped else "all"), "live": live, "shelves": shelves, "running": np.arange(ndata),
            "rows": rows, "cap": None}


def dense_cases():
    return [dense_case(M, False) for M in DENSE_M] + [dense_case(M, True) for M in DENSE_M if M < 300]


def dense_chunk(ref, rows, B, acceptable):
    """L [B, M]: nobody acceptable -- every value exactly on its threshold, one ulp below it, NaN or -inf -- but the
    candidates ``acceptable``, whose rows hold, data set by data set: the threshold itself, one ulp above it, +inf,
    and a value below, on and above the next value up of live + shelf."""
    rows = np.arange(ref.ndata) if rows is None else rows
    thr = ref.higher[rows]
    M = len(rows)
    which = (np.arange(B)[:, None] + np.arange(M)[None, :]) % 4
    thr2 = np.broadcast_to(thr, (B, M))
    L = np.select([which == 0, which == 1, which == 2], [thr2, np.nan, -np.inf], np.nextafter(thr2, -np.inf))
    for b in acceptable:
        for k, d in enumerate(rows):
            values = np.concatenate((ref.live[:, d], ref.shelf[d]))
            above = values[values > thr[k]]
            nxt = above.min() if len(above) else np.inf
            variant = (k + 1 + b) % 6
            if variant == 1:
                L[b, k] = np.nextafter(thr[k], np.inf)
            elif variant == 2:
                L[b, k] = np.inf
            elif variant == 3:
                L[b, k] = thr[k] + (nxt - thr[k]) / 2 if np.isfinite(nxt) and np.isfinite(thr[k]) else np.nextafter(thr[k], np.inf)
                if not L[b, k] > thr[k]:                   # (the next value up is one ulp away)
                    L[b, k] = nxt
            elif variant == 4:
                L[b, k] = nxt
            elif variant == 5:
                L[b, k] = nxt + 1.0
            else:
                L[b, k] = thr[k]
    return np.ascontiguousarray(L)


def run_dense_case(driver, case):
    """-> the reference after all chunks (``seen`` holds the COMMIT_KINDS that occurred)"""
    ref = planted_state(driver, case)
    compare_prepare(driver, ref, case["name"])
    ref.seen.clear()
    rows = case["rows"]
    sel = np.arange(ref.ndata) if rows is None else rows
    for B, acceptable in DENSE_CHUNKS:
        L = dense_chunk(ref, rows, B, acceptable)
        open_before = (ref.higher[sel] < np.inf).any()
        idx, beats = compare_chunk(driver, ref, L, rows, (case["name"], B, acceptable))
        if not acceptable or not open_before:
            assert idx == -1
        else:
            assert idx in acceptable
            if idx == acceptable[0]:
                ref.seen.add(("first", B, idx))
    return ref


def check_dense_coverage(seen):
    """the non-vacuity conditions of the dense cases, on what the REFERENCE found"""
    assert seen >= set(COMMIT_KINDS), set(COMMIT_KINDS) - seen
    for B, acceptable in DENSE_CHUNKS:
        if acceptable:
            assert ("first", B, acceptable[0]) in seen, (B, acceptable)
