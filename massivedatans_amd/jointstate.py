"""The floating-point state of the joint sampler behind one interface, twice.

The reference keeps the likelihoods of all live points (``live_pointsL[nlive, ndata]``,
multi_nested_sampler.py:111) and of the accepted points waiting on the shelves (:117) in
Python, and derives from them on every draw the thresholds ``Lmins_higher`` (:438-447), the
accept test ``any(L > Lmins)`` (hiermetriclearn.py:193) and the shelf fill (:482-485).  The
sampler of this package can hand all of that to a *joint state* object and keep only the
integer side (point ids, queues of ids, the data-set graph):

* :class:`DeviceJointState` -- the state lives in HBM behind an ``mdns_joint`` handle (``mdns_joint_*``
  of include/mdns.h); a draw chunk is scored, decided and committed on the GPU and only the accepted
  candidate's index and fill bits come back.  Its three kinds differ in how the initial points are
  scored and how a chunk is handed over:

  - :class:`GaussJointState` -- the Gaussian line, from the parameters (optionally with the
    accepted candidate's likelihood row);
  - :class:`MuseJointState` -- the MUSE-style lines, from the parameters;
  - :class:`CurveJointState` -- a model the CALLER evaluates: a Python function makes one model curve
    per candidate (numpy, or a torch tensor on the device), or a table on the device does; the device
    does everything after the curves.
* :class:`HostJointState` -- the same interface in numpy over any ``loglike_batch`` scorer.  It
  is the statement the device implementation is tested against (tests/), and what the CPU
  tests run the orchestration with.

Interface (``rows`` are ORIGINAL data-set indices, ascending; ``running`` likewise):

    init(xs)                     score the initial live points (physical parameter rows)
    set_running(running)         the data sets still being sampled (cut_down)
    prepare() -> Lmin, argmin, keep     start of an iteration; keep[r, e] = shelf entry e of the
                                        r-th running data set stays (bool matrix as wide as the
                                        longest shelf; None when nothing was dropped anywhere)
    draw(xs, rows) -> idx, Lrow, beats, nscored
                                 first acceptable candidate of the chunk (or -1), its
                                 likelihoods over ``rows``, which of them it beats; the state
                                 takes the point in; ``nscored`` candidates were looked at
    advance()                    end of an iteration
    live_matrix() -> L[nlive, nrunning]

The chunk in two halves, for whoever reduces the candidates' votes over several states in between
(``parallel.ShardedJointState``: one state per rank, each over its block of the data sets):

    score_backend(params, rows, jitter=None)     scores the chunk (kernel parameter rows): one 0 / 1 vote
                                                 per candidate, 1 where a selected data set accepts it
    votes() -> int32[B]          set_votes(v)    (device states also: votes_address(), to reduce in place)
    commit_backend() -> idx, Lrow or None, beats     the first candidate with a vote (-1: none) is taken in
                                                     by the data sets of THIS state it beats
"""
import ctypes as C

import numpy

from . import _host, _lib


class HostJointState(object):
    """numpy statement of the joint state over ``scorer.loglike_batch(params[B, 3], mask)``
    (``params`` rows are (A, mu, sig), ``mask`` a bool array over all data sets)."""

    #: candidates scored at once grow 1, 2, 4 ... up to this (a CPU scorer pays per candidate)
    MAX_CHUNK = 64

    def __init__(self, scorer, nlive, ndata, to_kernel_params, nparams=3):
        self.scorer = scorer
        self.nlive, self.ndata = int(nlive), int(ndata)
        self.to_kernel_params = to_kernel_params
        self.nparams = int(nparams)
        self.live = None                                  # [nlive, ndata], all data sets ever
        self.shelfL = [[] for _ in range(self.ndata)]
        self.higher = numpy.full(self.ndata, numpy.nan)
        self.running = numpy.arange(self.ndata)
        self.argmin = numpy.zeros(self.ndata, dtype=int)
        self.nevals_scored = 0
        self.ncalls = 0

    def init(self, xs, jitter=None):
        """``jitter`` [nlive, ndata]: noise added to the likelihoods (musefuse.py:535)."""
        self.live = numpy.array(self.scorer.loglike_batch(self.to_kernel_params(xs), numpy.ones(self.ndata, dtype=bool)))
        if jitter is not None:
            self.live = self.live + jitter
        self.nevals_scored += self.live.size
        self.ncalls += 1
        assert self.live.shape == (self.nlive, self.ndata)

    def set_running(self, running):
        self.running = numpy.asarray(running, dtype=int)

    def _threshold(self, d):
        n = len(self.shelfL[d])
        merged = numpy.concatenate((self.live[:, d], self.shelfL[d]))
        return numpy.partition(merged, n)[n]              # find_nsmallest, multi_nested_sampler.py:44-47

    def prepare(self):
        run = self.running
        cols = self.live[:, run]
        Lmin = cols.min(axis=0)
        arg = cols.argmin(axis=0)
        self.argmin[run] = arg
        width = max([len(self.shelfL[d]) for d in run] + [0])
        keep = numpy.zeros((len(run), width), dtype=bool)
        dropped = False
        for r, d in enumerate(run):
            k = [L > Lmin[r] for L in self.shelfL[d]]
            dropped = dropped or not all(k)
            keep[r, :len(k)] = k
            self.shelfL[d] = [L for L, kk in zip(self.shelfL[d], k) if kk]
            self.higher[d] = self._threshold(d) if self.shelfL[d] else Lmin[r]
        return Lmin, arg, (keep if dropped else None)

    def chunk_size(self, offered, M, hint=None):
        return offered

    def took(self, rows, beats):
        """(a native constrainer's draw ended in this state's ``draw_params``: nothing to add)"""

    def draw(self, xs, rows):
        return self.draw_params(self.to_kernel_params(xs), rows)

    def draw_params(self, params, rows, jitter=None):
        """``draw`` for candidates given as kernel parameter rows; ``jitter`` [B, M] is added to
        their likelihoods before anything is compared or kept."""
        rows = numpy.arange(self.ndata) if rows is None else numpy.asarray(rows, dtype=int)
        mask = numpy.zeros(self.ndata, dtype=bool)
        mask[rows] = True
        thr = self.higher[rows]
        pos, chunk = 0, 1
        while pos < len(params):
            Ls = self.scorer.loglike_batch(params[pos:pos + chunk], mask)
            if jitter is not None:
                Ls = Ls + jitter[pos:pos + len(Ls)]
            self.nevals_scored += Ls.size
            self.ncalls += 1
            ok = (Ls > thr).any(axis=1)
            if ok.any():
                i = int(numpy.argmax(ok))
                Lrow = Ls[i]
                beats = Lrow > thr
                for d, L in zip(rows[beats], Lrow[beats]):
                    self.shelfL[d].append(L)
                    self.higher[d] = self._threshold(d)
                return pos + i, Lrow, beats, pos + i + 1
            pos += len(Ls)
            chunk = min(self.MAX_CHUNK, 2 * chunk)
        return -1, None, None, len(params)

    # the two halves of draw(), for a host that reduces the accept flags over several states
    # (parallel.ShardedJointState) in between
    def score(self, xs, rows):
        """Accept flag of every candidate of the chunk against the selected data sets."""
        return self.score_params(self.to_kernel_params(xs) if len(xs) else numpy.zeros((0, self.nparams)), rows)

    def score_params(self, params, rows, jitter=None):
        """``score`` for candidates given as kernel parameter rows; ``jitter`` [B, M] is added to the
        likelihoods before anything is compared or kept (musefuse.py:535)."""
        xs = params
        rows = numpy.arange(self.ndata) if rows is None else numpy.asarray(rows, dtype=int)
        self._scored_rows = rows
        if len(rows) == 0 or len(xs) == 0:
            self._scored_L = numpy.zeros((len(xs), 0))
            return numpy.zeros(len(xs), dtype=numpy.int32)
        mask = numpy.zeros(self.ndata, dtype=bool)
        mask[rows] = True
        self._scored_L = self.scorer.loglike_batch(params, mask)
        if jitter is not None:
            self._scored_L = self._scored_L + numpy.asarray(jitter)[:len(self._scored_L)]
        self.nevals_scored += self._scored_L.size
        self.ncalls += 1
        return (self._scored_L > self.higher[rows]).any(axis=1).astype(numpy.int32)

    def commit(self, idx):
        """Candidate ``idx`` of the scored chunk is the accepted point: its likelihoods over the
        scored selection, which data sets it beats; those take it in."""
        rows = self._scored_rows
        Lrow = self._scored_L[idx]
        beats = Lrow > self.higher[rows]
        for d, L in zip(rows[beats], Lrow[beats]):
            self.shelfL[d].append(L)
            self.higher[d] = self._threshold(d)
        return Lrow, beats

    # the same two halves as every state speaks them (module docstring): the votes are the accept flags
    def score_backend(self, params, rows, jitter=None):
        self._votes = self.score_params(params, rows, jitter=jitter)

    def votes(self):
        return self._votes

    def set_votes(self, votes):
        self._votes = numpy.asarray(votes, dtype=numpy.int32)

    def commit_backend(self):
        hit = numpy.flatnonzero(self._votes)
        if len(hit) == 0:
            return -1, None, numpy.zeros(len(self._scored_rows), dtype=bool)
        return (int(hit[0]),) + self.commit(int(hit[0]))

    def advance(self):
        for d in self.running:
            self.live[self.argmin[d], d] = self.shelfL[d].pop(0)

    def live_matrix(self):
        return self.live[:, self.running]

    def thresholds(self):
        return self.higher.copy(), numpy.array([len(s) for s in self.shelfL])


def pack_fill_bits(beats):
    """Fill bits as the library keeps them: bit ``k`` of the uint64 words = ``beats[k]``."""
    words = numpy.zeros((len(beats) + 63) // 64, dtype=numpy.uint64)
    packed = numpy.packbits(numpy.asarray(beats, dtype=numpy.uint8), bitorder='little')
    words.view(numpy.uint8)[:len(packed)] = packed
    return words


def unpack_fill_bits(words, M):
    """The first ``M`` fill bits of ``words`` (uint64) as a bool vector."""
    return numpy.unpackbits(words[:(M + 63) // 64].view(numpy.uint8), bitorder='little')[:M].astype(bool)


class DeviceJointState(object):
    """A joint state in HBM behind an ``mdns_joint`` handle on ``spectra`` (include/mdns.h Part 2b): what every
    kind of it does the same way.  A kind adds ``init`` and, where its chunks are not kernel parameter rows
    through the entry points a native constrainer calls (``mdns_backend_draw_*``), its own ``draw_params``."""

    nparams = 3
    #: the accepted candidate's likelihood row comes to the host with every draw (GaussJointState can)
    fetch_rows = False
    #: draws go through the entry points a native constrainer calls (GaussJointState has another route)
    via_backend = True

    def __init__(self, spectra, nlive, to_kernel_params, shelf_cap=64):
        self._nscored = C.c_int(0)
        self._lib = _lib.require_device()
        self.spectra = spectra                             # keeps the spectra handle alive
        self.nlive, self.ndata = int(nlive), int(spectra.ndata)
        self.noise_level = float(getattr(spectra, "noise_level", 0.0))
        self.to_kernel_params = to_kernel_params
        self._h = self._lib.mdns_joint_create(spectra.handle, self.nlive, int(shelf_cap))
        if not self._h:
            raise _lib.MdnsError("mdns_joint_create failed: " + _lib.last_error())
        self.running = numpy.arange(self.ndata, dtype=numpy.int32)
        self.shelf_n = numpy.zeros(self.ndata, dtype=numpy.int64)     # mirror of the device's shelf sizes
        self.cap = self._lib.mdns_joint_shelf_cap(self._h)
        self._bits = numpy.zeros((self.ndata + 63) // 64, dtype=numpy.uint64)
        self._accepted = C.c_int(-1)
        self.nevals_scored = 0
        self.ncalls = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mdns_joint_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.MdnsError("%s failed: %s" % (what, _lib.last_error()))

    def _beats(self, M):
        """The fill bits the last outcome left in ``_bits``: which of the ``M`` selected data sets the point beats."""
        return unpack_fill_bits(self._bits, M)

    def _init_jitter(self, jitter):
        """The noise block ``init`` adds to the initial points' likelihoods, checked (None stays None)."""
        if jitter is not None:
            jitter = _lib.as_f64(jitter)
            if jitter.shape != (self.nlive, self.ndata):
                raise ValueError("jitter must be [nlive, ndata]")
        return jitter

    def _initialised(self):
        """(the end of every ``init``: empty shelves, nlive x ndata pairs scored)"""
        self.shelf_n[:] = 0
        self.nevals_scored += self.nlive * self.ndata
        self.ncalls += 1

    def set_running(self, running):
        self.running = numpy.ascontiguousarray(running, dtype=numpy.int32)
        self._check(self._lib.mdns_joint_set_running(self._h, _lib.ptr(self.running), len(self.running)),
                    "mdns_joint_set_running")

    def prepare(self):
        n = len(self.running)
        kw = self._lib.mdns_joint_keep_words(self._h)
        Lmin = numpy.empty(n)
        arg = numpy.empty(n, dtype=numpy.int32)
        keepw = numpy.empty((n, kw), dtype=numpy.uint64)
        self._check(self._lib.mdns_joint_prepare(self._h, _lib.ptr(Lmin), _lib.ptr(arg), _lib.ptr(keepw)),
                    "mdns_joint_prepare")
        counts = self.shelf_n[self.running]
        keep = None
        if counts.any():
            # kept entries per data set = set bits; anything dropped shows as a smaller count
            kept = numpy.zeros(n, dtype=numpy.int64)
            for w in range(kw):
                kept += _popcount(keepw[:, w])
            if (kept != counts).any():
                width = int(counts.max())
                keep = numpy.zeros((n, width), dtype=bool)
                for e in range(width):
                    keep[:, e] = (keepw[:, e // 64] >> numpy.uint64(e % 64)) & numpy.uint64(1)
                self.shelf_n[self.running] = kept
        return Lmin, arg.astype(int), keep

    def chunk_size(self, offered, M, hint=None):
        """How many of the offered candidates one chunk scores (the library's own choice)."""
        return int(self._lib.mdns_backend_chunk_size(self._h, int(offered), int(M), int(hint or 1)))

    def took(self, rows, beats):
        """A point went onto the shelves of ``rows[beats]`` (``rows`` None: of ``beats``): the mirror of the
        sizes follows.  A parameter draw of this state says so itself; whoever reaches the handle another
        way -- a native constrainer (mdns_backend_draw_chunk), a test -- calls this."""
        if rows is None:
            self.shelf_n[beats] += 1
        else:
            self.shelf_n[rows[beats]] += 1

    def _selection(self, rows):
        """``rows`` as the library takes a selection, and how many data sets it names."""
        if rows is None:
            return None, self.ndata
        rows = numpy.ascontiguousarray(rows, dtype=numpy.int32)
        return rows, len(rows)

    def _outcome(self, B, M):
        """What a chunk handed over another way than :meth:`draw_params` left: ``(idx, None, beats, B)`` as ``draw``
        answers (whether the point counts into the mirror is the caller's)."""
        self.ncalls += 1
        self.nevals_scored += B * M
        idx = self._accepted.value
        if idx < 0:
            return -1, None, None, B
        return idx, None, self._beats(M), B

    def draw(self, xs, rows):
        return self.draw_params(self.to_kernel_params(xs[:_lib.JOINT_MAX_BATCH]), rows)

    def draw_params(self, params, rows, jitter=None):
        """``draw`` for candidates given as kernel parameter rows, through the entry points a native constrainer
        calls (mdns_backend_draw_begin / mdns_backend_draw_chunk; no likelihood row); ``jitter`` [B, M] is added
        to their likelihoods before anything is compared or kept.  (Every chunk of a run that is not a native
        constrainer's own comes through here: the steps stand in line, without helpers.)"""
        M = self.ndata if rows is None else len(rows)
        B = min(len(params), _lib.JOINT_MAX_BATCH)
        if B == 0 or M == 0:
            return -1, None, None, B
        params = _lib.as_f64(params[:B])
        if rows is not None:
            rows = numpy.ascontiguousarray(rows, dtype=numpy.int32)
        if jitter is not None:
            jitter = _lib.as_f64(jitter)
        self._check(self._lib.mdns_backend_draw_begin(self._h, _lib.opt(rows), M), "mdns_backend_draw_begin")
        self._check(self._lib.mdns_backend_draw_chunk(self._h, _lib.ptr(params), B, _lib.opt(jitter), C.addressof(self._accepted),
                                                      _lib.ptr(self._bits), C.addressof(self._nscored)),
                    "mdns_backend_draw_chunk")
        self.ncalls += 1
        self.nevals_scored += B * M
        idx = self._accepted.value
        if idx < 0:
            return -1, None, None, B
        beats = self._beats(M)
        self.took(rows, beats)
        return idx, None, beats, B

    # the two halves of a chunk (include/mdns.h: mdns_backend_draw_score / mdns_backend_draw_commit): what
    # parallel.ShardedJointState puts the MAX all-reduce of the candidates' votes between
    def score_backend(self, params, rows, jitter=None):
        """Scores the chunk against the selected data sets ``rows`` (ORIGINAL indices of this state's
        spectra, ascending; None: all); one 0 / 1 vote per candidate stays on the device
        (:meth:`votes_address`)."""
        B = len(params)
        if B > _lib.JOINT_MAX_BATCH:
            raise ValueError("at most %d candidates per chunk" % _lib.JOINT_MAX_BATCH)
        rows, M = self._selection(rows)
        params = _lib.as_f64(params) if B else None
        if jitter is not None:
            jitter = _lib.as_f64(jitter)
            if jitter.shape != (B, M):
                raise ValueError("jitter must be [B, M]")
        self._check(self._lib.mdns_backend_draw_begin(self._h, _lib.opt(rows if M else None), M), "mdns_backend_draw_begin")
        self._check(self._lib.mdns_backend_draw_score(self._h, _lib.opt(params), B, _lib.opt(jitter if B * M else None)),
                    "mdns_backend_draw_score")
        self._half = (rows, M, B)
        self.nevals_scored += B * M
        self.ncalls += 1

    def votes_address(self):
        return self._lib.mdns_joint_votes_dev(self._h)

    def votes(self):
        rows, M, B = self._half
        out = numpy.zeros(B, dtype=numpy.int32)
        if B:
            self._check(self._lib.mdns_d2h(_lib.ptr(out), self.votes_address(), out.nbytes), "mdns_d2h")
        return out

    def set_votes(self, votes):
        votes = numpy.ascontiguousarray(votes, dtype=numpy.int32)
        if len(votes):
            self._check(self._lib.mdns_h2d(self.votes_address(), _lib.ptr(votes), votes.nbytes), "mdns_h2d")

    def commit_backend(self):
        """The first candidate that has a vote now is the accepted point: (its index or -1, None -- no
        likelihood row leaves the device --, which of the selected data sets of THIS state it beats)."""
        rows, M, B = self._half
        self._check(self._lib.mdns_backend_draw_commit(self._h, C.addressof(self._accepted), _lib.ptr(self._bits)),
                    "mdns_backend_draw_commit")
        idx = self._accepted.value
        if idx < 0 or M == 0:
            return idx, None, numpy.zeros(M, dtype=bool)
        beats = self._beats(M)
        self.took(rows, beats)
        return idx, None, beats

    def _reserve_for(self, rows):
        """Room on the device's shelves for one more point on the fullest shelf of ``rows`` (by the mirror of the sizes)."""
        nmax = int(self.shelf_n.max()) if rows is None else (int(self.shelf_n[rows].max()) if len(rows) else 0)
        if nmax + 1 > self.cap:
            self._check(self._lib.mdns_joint_reserve(self._h, nmax + 1), "mdns_joint_reserve")
            self.cap = self._lib.mdns_joint_shelf_cap(self._h)

    def advance(self):
        self._check(self._lib.mdns_joint_advance(self._h), "mdns_joint_advance")
        self.shelf_n[self.running] -= 1

    def live_matrix(self):
        full = numpy.empty((self.nlive, self.ndata))
        self._check(self._lib.mdns_joint_get_live(self._h, _lib.ptr(full)), "mdns_joint_get_live")
        if len(self.running) == self.ndata:
            return full
        return full[:, self.running]

    def thresholds(self):
        higher = numpy.empty(self.ndata)
        n = numpy.empty(self.ndata, dtype=numpy.int32)
        self._check(self._lib.mdns_joint_get_thresholds(self._h, _lib.ptr(higher), _lib.ptr(n)), "mdns_joint_get_thresholds")
        return higher, n.astype(int)


class GaussJointState(DeviceJointState):
    """The joint state of the Gaussian-line problem on the GPU, bound to a
    :class:`massivedatans_amd.like.GaussLineSpectra`."""

    #: (candidate, spectrum) pairs scored per chunk at most: ~50 us of GPU time
    EVAL_BUDGET = 2560000
    MIN_CHUNK = 32

    def __init__(self, spectra, nlive, to_kernel_params, shelf_cap=64, fetch_rows=True, via_backend=False):
        super(GaussJointState, self).__init__(spectra, nlive, to_kernel_params, shelf_cap=shelf_cap)
        #: copy the accepted candidate's likelihood row to the host with every draw (the sampler
        #: itself needs only the index and the fill bits: sample.py turns this off)
        self.fetch_rows = fetch_rows
        #: make ``draw`` go through the entry points a native constrainer calls
        #: (mdns_backend_draw_begin / mdns_backend_draw_chunk; no likelihood row) -- tests
        self.via_backend = via_backend
        self._Lrow = numpy.empty(self.ndata)

    def init(self, xs):
        params = _lib.as_f64(self.to_kernel_params(xs))
        if params.shape != (self.nlive, 3):
            raise ValueError("initial points must be [nlive, 3]")
        self._check(self._lib.mdns_joint_init_gauss(self._h, _lib.ptr(params), self.noise_level), "mdns_joint_init_gauss")
        self._initialised()

    def chunk_size(self, offered, M, hint=None):
        """How many of the offered candidates one launch scores: four times the tries the last
        draw needed (``hint``), within a budget of (candidate, spectrum) pairs."""
        budget = max(self.MIN_CHUNK, self.EVAL_BUDGET // max(1, M))
        if hint is not None:
            budget = min(budget, max(self.MIN_CHUNK, 4 * int(hint)))
        return int(min(offered, budget, _lib.JOINT_MAX_BATCH))

    def draw_params(self, params, rows, jitter=None):
        """``draw`` for candidates given as kernel parameter rows (A, mu, sig): through the backend entry points
        (``via_backend``), or in one call that can hand the likelihood row over (mdns_joint_draw_gauss)."""
        if self.via_backend:
            return DeviceJointState.draw_params(self, params, rows, jitter)
        if jitter is not None:
            raise ValueError("likelihood jitter goes through the backend entry points")
        rows, M = self._selection(rows)
        B = min(len(params), _lib.JOINT_MAX_BATCH)
        params = _lib.as_f64(params[:B])
        self._reserve_for(rows)
        self._check(self._lib.mdns_joint_draw_gauss(
            self._h, _lib.ptr(params), B, self.noise_level, _lib.opt(rows), M,
            C.byref(self._accepted), _lib.opt(self._Lrow if self.fetch_rows else None), _lib.ptr(self._bits)),
            "mdns_joint_draw_gauss")
        idx, _, beats, _ = self._outcome(B, M)
        if idx < 0:
            return -1, None, None, B
        self.took(rows, beats)
        return idx, (self._Lrow[:M].copy() if self.fetch_rows else None), beats, B


class MuseJointState(DeviceJointState):
    """The joint state of the MUSE-style problem on the GPU: spectra with per-pixel variances
    (:class:`massivedatans_amd.like.MuseSpectra`), the template evaluated on the device from the
    parameters -- 5 of the built-in three lines, G + 2 of the spectra's line list --, the
    scale-marginalised likelihood of cmuselike.c:45-64."""

    def __init__(self, spectra, nlive, shelf_cap=64):
        super(MuseJointState, self).__init__(spectra, nlive, lambda xs: xs, shelf_cap=shelf_cap)
        self.nparams = int(self._lib.mdns_spectra_nparams(spectra.handle))

    def init(self, xs, jitter=None):
        params = _lib.as_f64(xs)
        if params.shape != (self.nlive, self.nparams):
            raise ValueError("initial points must be [nlive, %d]" % self.nparams)
        self._check(self._lib.mdns_joint_init_muse3(self._h, _lib.ptr(params), _lib.opt(self._init_jitter(jitter))),
                    "mdns_joint_init_muse3")
        self._initialised()


class CurveJointState(DeviceJointState):
    """The joint state of a caller-defined model on the GPU.  ``model(xs f64[B, ndim]) -> curves [B, nx]``
    makes one model curve per candidate -- a C-contiguous float64 numpy array, or a float64 torch tensor
    on the device the library runs on, which is then read where it lies (by pointer and row stride; nothing
    is copied through the host) -- and the device scores, decides and commits from the curves
    (``mdns_backend_draw_curves[_dev]``, include/mdns.h).  Over a
    :class:`massivedatans_amd.like.GaussLineSpectra` the likelihood is the fixed-noise one of sample.py:64-71
    at the spectra's ``noise_level``, over a :class:`massivedatans_amd.like.MuseSpectra` the
    scale-marginalised one of cmuselike.c:45-64, over a :class:`massivedatans_amd.like.WeightedSpectra` the
    fixed-scale one with per-pixel variances (mdns_curve_chi2_batch), over a
    :class:`massivedatans_amd.like.CountSpectra` the Poisson one (mdns_curve_poisson_batch; with a background the W
    statistic, mdns_curve_wstat_batch).  ``nparams`` is the model's ``ndim``: what the first
    ``init`` is given, or ``ndim=``.  With ``table=`` (a :class:`massivedatans_amd.tablemodel.DeviceTable`, or a
    :class:`massivedatans_amd.summodel.DeviceSum`, which names its two entries) the curves are made on the device from the
    parameters and ``model`` is not called.

    A native constrainer reaches this state through ``constrainer.python_backend``, whose chunks end in
    :meth:`draw_params`.  A curve chunk does not count its point into ``shelf_n``: whoever drives the draws
    -- the sampler, the native core, a test -- may or may not do so itself (:meth:`took`), so
    :meth:`prepare` reads the shelf sizes back from the device instead of trusting the mirror."""

    def __init__(self, spectra, nlive, model, shelf_cap=64, ndim=None, table=None):
        super(CurveJointState, self).__init__(spectra, nlive, lambda xs: xs, shelf_cap=shelf_cap)
        self.model = model
        self.nx = int(spectra.nx)
        # what a model curve holds: the bins of the spectra's response, or -- without one -- the channels
        self.n_in = int(getattr(spectra, "n_in", spectra.nx))
        self.nparams = int(ndim) if ndim is not None else None
        # a table model on the device (tablemodel.DeviceTable): init and draw_params hand it the parameters and
        # ``model`` is never called (mdns_joint_init_table, mdns_backend_draw_table)
        self.table = table
        if table is not None:
            if self.nparams is not None and self.nparams != table.ndim:
                raise ValueError("ndim = %d, the table model takes %d parameters" % (self.nparams, table.ndim))
            self.nparams = int(table.ndim)
        # the two entries that take the device model's handle: the object's own (summodel.DeviceSum), or the table's
        self._init_entry = getattr(table, "init_entry", "mdns_joint_init_table")
        self._draw_entry = getattr(table, "draw_entry", "mdns_backend_draw_table")
        self._d_jitter, self._d_jitter_bytes = None, 0
        self._n32 = numpy.zeros(self.ndata, dtype=numpy.int32)

    def close(self):
        if getattr(self, "_d_jitter", None):
            self._lib.mdns_dev_free(self._d_jitter)
            self._d_jitter = None
        super(CurveJointState, self).close()

    def _curves(self, xs):
        """``model(xs)`` as ``(address, row stride in doubles, on the device?, what keeps it alive)``."""
        n = len(xs)
        curves = self.model(xs)
        if hasattr(curves, "data_ptr") and getattr(curves, "is_cuda", False):
            import torch
            if curves.dtype != torch.float64 or curves.dim() != 2 or tuple(curves.shape) != (n, self.n_in):
                raise ValueError("the model must return float64 curves [%d, %d], got %s %s"
                                 % (n, self.n_in, curves.dtype, tuple(curves.shape)))
            if curves.stride(1) != 1 or (n > 1 and curves.stride(0) < self.n_in):
                curves = curves.contiguous()
            # the library reads on its own stream: what torch has queued for the tensor must be done
            torch.cuda.current_stream(curves.device).synchronize()
            return curves.data_ptr(), max(int(curves.stride(0)), self.n_in), True, curves
        if hasattr(curves, "detach"):                     # a host tensor
            curves = curves.detach().numpy()
        curves = _lib.as_f64(curves)
        if curves.shape != (n, self.n_in):
            raise ValueError("the model must return curves [%d, %d], got %s" % (n, self.n_in, curves.shape))
        return _lib.ptr(curves), self.n_in, False, curves

    def init(self, xs, jitter=None):
        xs = numpy.asarray(xs, dtype=float)
        if xs.ndim != 2 or len(xs) != self.nlive or (self.nparams is not None and xs.shape[1] != self.nparams):
            raise ValueError("initial points must be [nlive, ndim]")
        self.nparams = int(xs.shape[1])
        jitter = self._init_jitter(jitter)
        if self.table is not None:
            xs = _lib.as_f64(xs)
            init = getattr(self._lib, self._init_entry)
            self._check(init(self._h, self.table.handle, _lib.ptr(xs), self.noise_level, _lib.opt(jitter)), self._init_entry)
        else:
            address, ld, on_device, keep = self._curves(xs)
            if on_device:                                     # (once per run: through the host)
                keep = _lib.as_f64(keep.cpu().numpy())
                address = _lib.ptr(keep)
            self._check(self._lib.mdns_joint_init_curves(self._h, address, self.noise_level, _lib.opt(jitter)), "mdns_joint_init_curves")
        self._initialised()

    def prepare(self):
        self._check(self._lib.mdns_joint_get_thresholds(self._h, None, _lib.ptr(self._n32)), "mdns_joint_get_thresholds")
        self.shelf_n[:] = self._n32
        return super(CurveJointState, self).prepare()

    def draw_params(self, params, rows, jitter=None):
        """One chunk: ``params[B, ndim]`` as the model takes them (at most ``MDNS_JOINT_MAX_BATCH`` are
        looked at); ``jitter`` [B, M] is added to the likelihoods before anything is compared or kept."""
        rows, M = self._selection(rows)
        B = min(len(params), _lib.JOINT_MAX_BATCH)
        if B == 0 or M == 0:
            return -1, None, None, B
        params = numpy.asarray(params, dtype=float)[:B]
        if self.table is not None:
            params = _lib.as_f64(params)
            if params.ndim != 2 or params.shape[1] != self.table.ndim:
                raise ValueError("params must be [B, %d], got %s" % (self.table.ndim, params.shape))
            address, ld, on_device, keep = None, self.n_in, False, params
        else:
            address, ld, on_device, keep = self._curves(params)
        if jitter is not None:
            jitter = _lib.as_f64(jitter)[:B]
            if jitter.shape != (B, M):
                raise ValueError("jitter must be [B, M]")
        self._check(self._lib.mdns_backend_draw_begin(self._h, _lib.opt(rows), M), "mdns_backend_draw_begin")
        out = (C.addressof(self._accepted), _lib.ptr(self._bits), C.addressof(self._nscored))
        if self.table is not None:
            draw = getattr(self._lib, self._draw_entry)
            self._check(draw(self._h, self.table.handle, _lib.ptr(params), B, _lib.opt(jitter), *out), self._draw_entry)
        elif on_device:
            self._check(self._lib.mdns_backend_draw_curves_dev(self._h, address, ld, B, self._jitter_to_device(jitter), *out),
                        "mdns_backend_draw_curves_dev")
        else:
            self._check(self._lib.mdns_backend_draw_curves(self._h, address, B, _lib.opt(jitter), *out), "mdns_backend_draw_curves")
        del keep
        return self._outcome(B, M)

    def _jitter_to_device(self, jitter):
        """The noise block of a chunk whose curves are on the device already (a synchronous copy)."""
        if jitter is None:
            return None
        if jitter.nbytes > self._d_jitter_bytes:
            if self._d_jitter:
                self._check(self._lib.mdns_sync(), "mdns_sync")
                self._lib.mdns_dev_free(self._d_jitter)
            self._d_jitter_bytes = 2 * jitter.nbytes
            self._d_jitter = self._lib.mdns_dev_alloc(self._d_jitter_bytes)
            if not self._d_jitter:
                self._d_jitter_bytes = 0
                raise _lib.MdnsError("mdns_dev_alloc failed: " + _lib.last_error())
        self._check(self._lib.mdns_h2d(self._d_jitter, _lib.ptr(jitter), jitter.nbytes), "mdns_h2d")
        return self._d_jitter

    def draw_gauss_params(self, params, rows):
        """A chunk of the built-in Gaussian line, ``params[B, 3]`` = (A, mu, sig), on this state (fixed-noise
        spectra only): parameter chunks and curve chunks may alternate."""
        return DeviceJointState.draw_params(self, params, rows)


_POP8 = numpy.array([bin(i).count("1") for i in range(256)], dtype=numpy.int64)


def _popcount(words):
    """Set bits of every uint64 of ``words``."""
    if hasattr(numpy, "bitwise_count"):
        return numpy.bitwise_count(numpy.ascontiguousarray(words)).astype(numpy.int64)
    return _POP8[numpy.ascontiguousarray(words).view(numpy.uint8).reshape(len(words), 8)].sum(axis=1)


__all__ = ['HostJointState', 'DeviceJointState', 'GaussJointState', 'MuseJointState', 'CurveJointState',
           'pack_fill_bits', 'unpack_fill_bits']
