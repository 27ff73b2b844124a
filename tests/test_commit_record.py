"""The record ``k_joint_prepare`` leaves per data set (``JointRecord``, csrc/mdns_internal.h: threshold, live values at
or below it, next live value above it) and its use by ``shelf_append``, on planted states against a numpy statement.

The statement is the reference's rule and nothing else: with n points waiting, the threshold of a data set is the
(n+1)-th smallest of live + shelf (+inf when there are not that many), recomputed from the two arrays after every
change.  A NaN is no value: it is never counted and never a threshold -- how both device passes treat it.  Every
comparison is exact: thresholds, shelf sizes, the live matrix, the fill words, and the shelves' contents read out in
order through advance.

Whether an append took the record or the scan cannot be seen from outside, so the sequences are built so that both
paths occur and a wrongly used record shows: appends that leave the threshold where it was (the minimum occurs two
and three times: the record stays good), appends that move it (the second append scans), and live matrices rewritten
behind a prepare -- advance, undo_advance, set_live, restore_live_dev -- with values for which the record of the old
column gives ANOTHER threshold than the new column; that they differ is asserted on the statement alone
(test_a_stale_record_would_show, no device)."""
import ctypes as C

import numpy as np
import pytest

import joint_planted_support as jp

NDATA = (1, 63, 64, 65, 257)
NLIVE = (5, 100, 130)                 # 130: values beyond the 128 a data set's sixteen lanes hold in registers
CAP = 8
SHAPES = [(nd, nl) for nd in NDATA for nl in NLIVE]
KINDS = ("twice", "thrice", "distinct", "one-nan", "shelf-equal", "all-nan", "twice-far")
LOWEST = 4.0


# ---------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------
def threshold(col, shelf):
    """the (len(shelf) + 1)-th smallest of live + shelf, NaN being no value; +inf when there are fewer"""
    values = np.concatenate((col, shelf))
    values = np.sort(values[~np.isnan(values)])
    return values[len(shelf)] if len(shelf) < len(values) else np.inf


class Statement(object):
    def __init__(self, live):
        self.live = np.array(live, dtype=np.float64)
        self.nlive, self.ndata = self.live.shape
        self.shelf = [np.zeros(0) for _ in range(self.ndata)]
        self.higher = np.full(self.ndata, np.nan)
        self.argmin = np.zeros(self.ndata, dtype=int)
        self.Lmin = np.zeros(self.ndata)
        self.running = np.arange(self.ndata)

    def sizes(self):
        return np.array([len(s) for s in self.shelf])

    def set_live(self, live):
        self.live = np.array(live, dtype=np.float64)
        self.shelf = [np.zeros(0) for _ in range(self.ndata)]

    def prepare(self):
        for d in self.running:
            col = self.live[:, d]
            real = col[~np.isnan(col)]
            m = real.min() if len(real) else np.inf
            at = np.flatnonzero(col == m)
            self.Lmin[d], self.argmin[d] = m, (at[0] if len(at) else 0)
            self.shelf[d] = self.shelf[d][self.shelf[d] > m]
            self.higher[d] = threshold(col, self.shelf[d])

    def chunk(self, L, rows):
        rows = np.arange(self.ndata) if rows is None else np.asarray(rows)
        with np.errstate(invalid="ignore"):
            ok = L > self.higher[rows]
        if not ok.any():
            return -1, None
        idx = int(np.argmax(ok.any(axis=1)))
        for d, v in zip(rows[ok[idx]], L[idx][ok[idx]]):
            self.shelf[d] = np.append(self.shelf[d], v)
            self.higher[d] = threshold(self.live[:, d], self.shelf[d])
        return idx, ok[idx]

    def advance(self):
        for d in self.running:
            self.live[self.argmin[d], d] = self.shelf[d][0]
            self.shelf[d] = self.shelf[d][1:]

    def undo_advance(self):
        for d in self.running:
            self.live[self.argmin[d], d] = self.Lmin[d]
            self.shelf[d] = np.zeros(0)


# ---------------------------------------------------------------------------------------
# planted columns and chunks
# ---------------------------------------------------------------------------------------
def planted_live(ndata, nlive, seed):
    """Column d is of kind KINDS[d % 7]: distinct even values from 10 up in random slots; the minimum LOWEST put two or
    three times ("twice-far": at the last two slots, beyond the registers when nlive = 130); one NaN; all NaN."""
    rng = np.random.RandomState(seed)
    live = np.empty((nlive, ndata))
    for d in range(ndata):
        col = 10.0 + 2.0 * rng.permutation(nlive)
        kind = KINDS[d % len(KINDS)]
        if kind == "twice":
            col[rng.choice(nlive, size=2, replace=False)] = LOWEST
        elif kind == "thrice":
            col[rng.choice(nlive, size=3, replace=False)] = LOWEST
        elif kind == "twice-far":
            col[-2:] = LOWEST
        elif kind == "one-nan":
            col[rng.randint(nlive)] = np.nan
        elif kind == "all-nan":
            col[:] = np.nan
        live[:, d] = col
    return live


def takers(ndata):
    """the data sets that can take a point (an all-NaN column has the threshold +inf)"""
    return np.flatnonzero(np.array([KINDS[d % len(KINDS)] != "all-nan" for d in range(ndata)]))


def planted_chunk(ref, rows, step, all_beat):
    """L [2, M]: candidate 0 beats nobody (every value on its threshold, or NaN), candidate 1 lies, data set by data
    set, one above the threshold (below the next value up: values are even), ON the next value up of live + shelf (a
    live value: the shelf then holds a value equal to a live one), one above that, or -- unless ``all_beat`` -- on the
    threshold itself (no append)."""
    rows = np.arange(ref.ndata) if rows is None else np.asarray(rows)
    thr = ref.higher[rows]
    L = np.empty((2, len(rows)))
    L[0] = np.where(np.arange(len(rows)) % 3 == 1, np.nan, thr)
    for k, d in enumerate(rows):
        values = np.concatenate((ref.live[:, d], ref.shelf[d]))
        with np.errstate(invalid="ignore"):
            above = values[values > thr[k]]
        nxt = above.min() if len(above) else np.inf
        variant = (d // len(KINDS) + d + step) % (3 if all_beat else 4)
        if not np.isfinite(thr[k]):
            L[1, k] = 1e300                                    # threshold +inf: nothing beats it
        elif variant == 0 or not np.isfinite(nxt):
            L[1, k] = thr[k] + 1.0
        elif variant == 1:
            L[1, k] = nxt
        elif variant == 2:
            L[1, k] = nxt + 1.0
        else:
            L[1, k] = thr[k]
    return np.ascontiguousarray(L)


def same(driver, ref, what):
    higher, n = driver.thresholds()
    assert np.array_equal(n, ref.sizes()), (what, "shelf sizes")
    assert np.array_equal(higher, ref.higher, equal_nan=True), (what, "thresholds", higher, ref.higher)
    assert np.array_equal(driver.live_matrix(), ref.live, equal_nan=True), (what, "live")


def prepare(driver, ref, what):
    ref.prepare()
    Lmin, arg, _ = driver.prepare()
    assert np.array_equal(Lmin, ref.Lmin[ref.running]) and np.array_equal(arg, ref.argmin[ref.running]), (what, "prepare")
    same(driver, ref, what)


def commit(driver, ref, rows, step, what, all_beat=False):
    """one planted chunk on both; -> who took the point"""
    L = planted_chunk(ref, rows, step, all_beat)
    idx, beats = ref.chunk(L, rows)
    got, words = driver.chunk(L, rows)
    assert got == idx, (what, "accepted", got, idx)
    if idx >= 0:
        assert idx == 1 and np.array_equal(words, jp.pack_bits(beats)), (what, "fill words")
    same(driver, ref, what)
    return beats


def read_out(driver, ref, what):
    """the shelves' contents, in order: advance -> live matrix -> prepare until every shelf is empty"""
    keep = ref.running
    while True:
        run = keep[ref.sizes()[keep] > 0]
        if len(run) == 0:
            break
        ref.running = run
        driver.set_running(run)
        ref.advance()
        driver.advance()
        prepare(driver, ref, (what, "read-out"))
    ref.running = keep
    driver.set_running(keep)


def set_running(driver, ref, running):
    ref.running = np.asarray(running)
    driver.set_running(ref.running)


def gapped(ndata, seed):
    """a selection with gaps (None for a single data set)"""
    if ndata < 3:
        return None
    rng = np.random.RandomState(seed)
    return np.sort(rng.choice(ndata, size=ndata - ndata // 3, replace=False)).astype(np.int32)


# ---------------------------------------------------------------------------------------
# dense commits (k_joint_commit_dense) on planted doubles
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ndata,nlive", SHAPES)
def test_dense_commits_on_planted_columns(ndata, nlive):
    live = planted_live(ndata, nlive, 1000 * ndata + nlive)
    driver = jp.DeviceDriver(nlive, ndata, shelf_cap=CAP)
    try:
        ref = Statement(live)
        every, some = np.arange(ndata), takers(ndata)

        # prepare -> commit
        set_running(driver, ref, every)
        driver.set_live(live)
        prepare(driver, ref, "one commit")
        assert (ref.higher[some] == np.nanmin(live[:, some], axis=0)).all() and (ref.higher[np.setdiff1d(every, some)] == np.inf).all()
        beats = commit(driver, ref, None, 0, "one commit")
        assert beats is not None and beats.any()
        read_out(driver, ref, "one commit")

        # prepare -> commit -> commit -> commit: second and third appends to the same data sets, thresholds that stay
        # (the record still answers) and thresholds that have moved (the scan), over all data sets and a selection
        ref.set_live(live)
        driver.set_live(live)
        prepare(driver, ref, "three commits")
        stayed = moved = 0
        for step, rows in enumerate((None, gapped(ndata, ndata), None)):
            before = ref.higher.copy()
            beats = commit(driver, ref, rows, step, ("three commits", step))
            took = (every if rows is None else rows)[beats]
            stayed += int((ref.higher[took] == before[took]).sum())
            moved += int((ref.higher[took] != before[took]).sum())
        assert moved > 0 and (stayed > 0 or ndata < 2), (stayed, moved)
        assert ndata < 7 or any(len(s) and np.isin(s, live[:, d]).any() for d, s in enumerate(ref.shelf)), "no shelf entry equals a live value"
        read_out(driver, ref, "three commits")

        # prepare -> commit -> advance -> commit, no prepare in between: the record describes the column of before the
        # advance (test_a_stale_record_would_show: where the minimum occurred twice it would keep the old threshold)
        ref.set_live(live)
        driver.set_live(live)
        set_running(driver, ref, some)
        prepare(driver, ref, "advance")
        beats = commit(driver, ref, some.astype(np.int32) if len(some) < ndata else None, 0, "advance", all_beat=True)
        assert beats.all()
        ref.advance()
        driver.advance()
        same(driver, ref, "advanced")
        commit(driver, ref, None, 1, "commit behind an advance", all_beat=True)
        read_out(driver, ref, "advance")

        # undo_advance -> prepare -> commit, twice over: the benchmark's cycle
        ref.set_live(live)
        driver.set_live(live)
        for cycle in range(3):
            prepare(driver, ref, ("cycle", cycle))
            beats = commit(driver, ref, None, cycle, ("cycle", cycle), all_beat=True)
            assert beats[some].all()
            commit(driver, ref, None, cycle + 1, ("cycle, second append", cycle))
            ref.advance()
            driver.advance()
            same(driver, ref, ("cycle, advanced", cycle))
            ref.undo_advance()
            driver.undo_advance()
            same(driver, ref, ("cycle, taken back", cycle))
        assert np.array_equal(ref.live, live, equal_nan=True)
    finally:
        driver.close()


# ---------------------------------------------------------------------------------------
# a stale record would show
# ---------------------------------------------------------------------------------------
def appended(col, shelf, thr, L, seen_col=None):
    """The threshold after L joins the shelf, as shelf_append computes it; ``seen_col``: the column the live part of
    the two answers is taken from (the record of a prepare that saw ANOTHER column)."""
    live = col if seen_col is None else seen_col
    values = np.concatenate((live[~np.isnan(live)], shelf))
    at_most = int((values <= thr).sum())
    above = values[values > thr]
    return thr if at_most >= len(shelf) + 2 else min(L, above.min() if len(above) else np.inf)


def test_a_stale_record_would_show():
    """On the statement alone: where the minimum occurred twice, the column behind an advance (one of the two replaced
    by the shelf head) gives another threshold than the record of the column before it; and a column whose second
    smallest value was lowered to the minimum (what the set_live / restore_live_dev sequences write) gives another
    threshold than the record of the original."""
    live = planted_live(65, 100, 7)
    ref = Statement(live)
    ref.prepare()
    differ = columns = 0
    for d in range(65):
        if KINDS[d % len(KINDS)] not in ("twice", "twice-far"):
            continue
        columns += 1
        old = live[:, d].copy()
        new = old.copy()
        new[ref.argmin[d]] = LOWEST + 1.0                      # the head of the shelf after a first append of LOWEST + 1
        L = LOWEST + 3.0
        fresh = appended(new, np.zeros(0), LOWEST, L)
        assert fresh == threshold(new, np.array([L]))
        differ += fresh != appended(new, np.zeros(0), LOWEST, L, seen_col=old)
    assert differ == columns == 19
    for d in range(65):
        if KINDS[d % len(KINDS)] != "distinct":
            continue
        old = live[:, d]
        new = lowered(live)[:, d]
        m = old.min()
        fresh = appended(new, np.zeros(0), m, m + 1.0)
        assert fresh == threshold(new, np.array([m + 1.0])) == m
        assert appended(new, np.zeros(0), m, m + 1.0, seen_col=old) == m + 1.0


def lowered(live):
    """``live`` with the second smallest value of every column put down to the minimum: the minimum, and so the
    threshold of an empty shelf, stays; how often it occurs does not"""
    out = np.array(live)
    for d in range(out.shape[1]):
        col = out[:, d]
        if np.isnan(col).all():
            continue
        order = np.argsort(col)                                # (NaN last)
        if len(col) > 1 and not np.isnan(col[order[1]]):
            col[order[1]] = col[order[0]]
    return out


# ---------------------------------------------------------------------------------------
# Gaussian-line states through mdns_joint_score_dev / mdns_joint_commit_bits_dev (k_joint_commit_trail, the mailbox)
# ---------------------------------------------------------------------------------------
class GaussDriver(object):
    """A ``GaussJointState`` driven through the device-pointer entry points the benchmark uses; likelihoods of the
    statement from the same lane kernel (chain_support.LaneScorer), so everything agrees exactly."""

    def __init__(self, ndata, nlive, seed):
        from massivedatans_amd import _lib, gen, jointstate, sample
        from massivedatans_amd.like import GaussLineSpectra
        from chain_support import LaneScorer
        self._lib_module, self.sample = _lib, sample
        self.ndata, self.nlive = ndata, nlive
        data = gen.horns(ndata)
        self.spectra = GaussLineSpectra(data["x"], data["y"], noise_level=0.01)
        self.scorer = LaneScorer(self.spectra)
        self.js = jointstate.GaussJointState(self.spectra, nlive, sample.kernel_params, shelf_cap=CAP, fetch_rows=False)
        self.lib, self.h = self.js._lib, self.js._h
        self.rng = np.random.RandomState(seed)
        self.js.init(sample.priortransform_batch(self.rng.uniform(size=(nlive, 3))))
        self.d_params = self.lib.mdns_dev_alloc(64 * 24)
        self.d_live = self.lib.mdns_dev_alloc(nlive * ndata * 8)
        self.bits = np.zeros((ndata + 63) // 64, dtype=np.uint64)

    def close(self):
        self.lib.mdns_dev_free(self.d_params)
        self.lib.mdns_dev_free(self.d_live)
        self.js.close()
        self.spectra.close()

    def check(self, rc, what):
        self._lib_module.check(rc, what)

    def candidates(self, faint):
        """-> kernel parameter rows [B, 3] and their likelihoods [B, ndata]"""
        cube = self.rng.uniform(size=(24, 3))
        cube[:, 0] *= faint
        params = np.ascontiguousarray(self.sample.kernel_params(self.sample.priortransform_batch(cube)))
        return params, self.scorer.loglike_batch(params, np.ones(self.ndata, dtype=bool))

    def chunk(self, params):
        """-> accepted index, fill words (None when nobody was accepted)"""
        ptr = self._lib_module.ptr
        self.check(self.lib.mdns_h2d(self.d_params, ptr(params), params.nbytes), "mdns_h2d")
        self.check(self.lib.mdns_joint_score_dev(self.h, self.d_params, len(params), 0.01, None, self.ndata), "mdns_joint_score_dev")
        self.check(self.lib.mdns_joint_commit_bits_dev(self.h, None, self.ndata), "mdns_joint_commit_bits_dev")
        accepted = C.c_int(-2)
        self.bits[:] = 0
        self.check(self.lib.mdns_joint_fetch(self.h, self.ndata, C.addressof(accepted), ptr(self.bits)), "mdns_joint_fetch")
        return accepted.value, (self.bits.copy() if accepted.value >= 0 else None)

    def set_running(self, running):
        self.js.set_running(running)

    def prepare(self):
        return self.js.prepare()

    def advance(self):
        self.check(self.lib.mdns_joint_advance(self.h), "mdns_joint_advance")

    def undo_advance(self):
        self.check(self.lib.mdns_joint_undo_advance_dev(self.h), "mdns_joint_undo_advance_dev")

    def set_live(self, live):
        live = np.ascontiguousarray(live)
        self.check(self.lib.mdns_joint_set_live(self.h, self._lib_module.ptr(live)), "mdns_joint_set_live")

    def restore_live(self, live):
        live = np.ascontiguousarray(live)
        self.check(self.lib.mdns_h2d(self.d_live, self._lib_module.ptr(live), live.nbytes), "mdns_h2d")
        self.check(self.lib.mdns_joint_restore_live_dev(self.h, self.d_live), "mdns_joint_restore_live_dev")

    def live_matrix(self):
        full = np.empty((self.nlive, self.ndata))
        self.check(self.lib.mdns_joint_get_live(self.h, self._lib_module.ptr(full)), "mdns_joint_get_live")
        return full

    def thresholds(self):
        return self.js.thresholds()


def gauss_commit(driver, ref, faint, what):
    params, L = driver.candidates(faint)
    idx, beats = ref.chunk(L, None)
    got, words = driver.chunk(params)
    assert got == idx, (what, "accepted", got, idx)
    if idx >= 0:
        assert np.array_equal(words, jp.pack_bits(beats)), (what, "fill words")
    same(driver, ref, what)
    return idx, beats


@pytest.mark.gpu
@pytest.mark.parametrize("ndata,nlive", SHAPES)
def test_gauss_line_commits_through_the_trail(ndata, nlive):
    driver = GaussDriver(ndata, nlive, 77 * ndata + nlive)
    try:
        live = driver.live_matrix()
        ref = Statement(live)
        every = np.arange(ndata)
        set_running(driver, ref, every)
        prepare(driver, ref, "start")

        # who takes the first accepted point of a chunk of faint lines: they run, the cycle below advances them
        params, L = driver.candidates(0.05)
        ok = L > ref.higher
        assert ok.any(), "no candidate beats a threshold"
        some = np.flatnonzero(ok[int(np.argmax(ok.any(axis=1)))])
        set_running(driver, ref, some)

        # undo_advance -> prepare -> commit (-> commit: second appends), twice over: the benchmark's cycle
        for cycle in range(3):
            prepare(driver, ref, ("cycle", cycle))
            idx, beats = ref.chunk(L, None)
            got, words = driver.chunk(params)
            assert got == idx and np.array_equal(words, jp.pack_bits(beats)) and np.array_equal(np.flatnonzero(beats), some)
            same(driver, ref, ("cycle", cycle))
            gauss_commit(driver, ref, 0.03, ("cycle, second append", cycle))
            ref.advance()
            driver.advance()
            same(driver, ref, ("cycle, advanced", cycle))
            if cycle == 0:
                # a commit behind the advance, without a prepare: the records are those of the columns before it
                gauss_commit(driver, ref, 0.02, "commit behind an advance")
            ref.undo_advance()
            driver.undo_advance()
            same(driver, ref, ("cycle, taken back", cycle))
        assert np.array_equal(ref.live, live)

        # set_live and restore_live_dev between prepare and commit: the thresholds stay those of the prepare (the
        # minimum is where it was), the columns hold it twice now -- test_a_stale_record_would_show
        set_running(driver, ref, every)
        for how in ("set_live", "restore_live_dev"):
            ref.set_live(live)
            driver.set_live(live)
            prepare(driver, ref, how)
            changed = lowered(live)
            ref.set_live(changed)
            (driver.set_live if how == "set_live" else driver.restore_live)(changed)
            same(driver, ref, (how, "rewritten"))
            idx, beats = ref.chunk(L, None)
            got, words = driver.chunk(params)
            assert got == idx and idx >= 0 and np.array_equal(words, jp.pack_bits(beats)), (how, "commit")
            same(driver, ref, (how, "commit"))
            assert (ref.higher[beats] == live.min(axis=0)[beats]).all(), "the minimum occurs twice: the threshold stays"
    finally:
        driver.close()
