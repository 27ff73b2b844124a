"""Test helpers of the two-launch draw chunk (test_chunk_shapes.py on the device, test_chunk_shapes_host.py on numpy
alone): the shape list, the rule that says which chunks take the route and which ``k_chunk_accept<NST>`` they launch,
the numpy statement of a draw of several chunks, and the sequences both files run -- the host file on the reference's
likelihoods and without a device, to show that what the device test asserts can happen.

Inputs, the ``np.longdouble`` reference, thresholds and the decision are those of filter_support.py."""
import ctypes as C
import os

import numpy as np

import filter_support as fs

#: live points of a planted state: the thresholds and two fillers nobody looks at (above every likelihood)
NLIVE = 3
FILLER = 1e300

#: (ndata, selection, nx, B), selections as filter_support.selection makes them.  What each shape is for:
CHUNK_SHAPES = [
    (1, None, 1, 1),           # the smallest chunk; ld = 2, seven padded channels of the only stage
    (63, None, 64, 3),         # <8> at its last stage count; M and B one short of a tile
    (65, "2/3", 65, 4),        # <16> at its first; gathered rows, M = 43; one full candidate tile
    (128, None, 128, 5),       # <16> at its last; M = 128: the last selection k_chunk_commit takes; B one past a tile
    (129, None, 129, 8),       # <26> at its first; M = 129: the first selection k_joint_commit_trail takes
    (200, "2/3", 208, 9),      # <26> at its last; M = 133
    (257, None, 209, 13),      # <32> at its first; M one past four tiles
    (130, "1/10", 256, 17),    # <32> at its last; sparse, M = 13
    (300, None, 257, 6),       # one channel more: classic route
    (1100, None, 200, 33),     # 18 tiles: the trail commit over several workgroups, the last one publishing; 9 candidate tiles
    (64, None, 200, 1024),     # the largest chunk over one tile: first_flagged over 1024 flags, 256 workgroups writing one tile's trail
    (4096, None, 7, 256),      # 4096 workgroups: at 16 * num_cus of a 256-CU device ...
    (4096, None, 7, 257),      # ... and past it (whatever the CU count, expected_route says which side a shape is on)
    (4097, None, 8, 8),        # more than 4096 spectra: two-launch with 8 candidates ...
    (4097, None, 8, 9),        # ... classic with 9
]
#: the shapes the halves run at: both commit kernels at their switch, the trail commit over several workgroups, 1024 votes
HALVES_SHAPES = [(128, None, 128, 5), (129, None, 129, 8), (1100, None, 200, 33), (64, None, 200, 1024)]
OFFSETS = (0.0, 3.0)


def selection_size(shape):
    ndata, sel, _, _ = shape
    return ndata if sel is None else (max(1, ndata * 2 // 3) if sel == "2/3" else max(2, ndata // 10))


# ---------------------------------------------------------------------------------------
# the expected route
# ---------------------------------------------------------------------------------------
def cols_nx(nx):
    """channels of a spectrum padded to whole stages of 8 (csrc/mdns_internal.h)"""
    return (nx + 7) // 8 * 8


def _atoll(text):
    """C ``atoll``: the leading integer of ``text``, 0 without one"""
    text = text.strip()
    n = 1 if text[:1] in ("+", "-") else 0
    while n < len(text) and text[n].isdigit():
        n += 1
    try:
        return int(text[:n])
    except ValueError:
        return 0


def expected_route(M, B, nx, num_cus):
    """``chunk_fits`` (csrc/mdns_chunk.hip) and the MDNS_CHUNK_PATH check of ``backend_score`` (csrc/mdns_joint.hip),
    restated: the start of the name ``mdns_profile_kernel(0)`` reports after a Gaussian-line chunk of B candidates over
    M selected spectra of nx channels, ``"k_chunk_accept<NST>"``, or None where the chunk takes the classic route.
    Reads the two switches as the library does, so it holds in whatever environment the process was started."""
    if os.environ.get("MDNS_CHUNK_PATH") == "classic":
        return None
    limit = os.environ.get("MDNS_CHUNK_GROUPS")
    most = _atoll(limit) if limit and _atoll(limit) > 0 else 16 * num_cus
    groups = -(-M // 64) * -(-B // 4)
    if cols_nx(nx) > 256 or (M > 4096 and B > 8) or groups > most:
        return None
    nst = cols_nx(nx) // 8
    return "k_chunk_accept<%d>" % (8 if nst <= 8 else 16 if nst <= 16 else 26 if nst <= 26 else 32)


def check_route(name, route):
    """``name``, what mdns_profile_kernel(0) reports, against ``expected_route``"""
    if route is None:
        assert name and not name.startswith("k_chunk_accept"), ("a chunk of the classic route was scored by", name)
    else:
        assert name.startswith(route), ("expected %s, scored by" % route, name)


#: hipDeviceAttributeMultiprocessorCount of hip_runtime_api.h (part of the runtime's binary interface)
_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63


def device_cus(lib):
    """The device's multiprocessor count, the property the library sizes ``chunk_fits`` with (mdns_core.hip), asked of
    the HIP runtime the library itself is linked to and has initialised: in this process, no second runtime."""
    from massivedatans_amd import _lib
    _lib.require_device()
    ask = lib.hipDeviceGetAttribute
    ask.restype, ask.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int]
    device, count = C.c_int(-1), C.c_int(0)
    assert lib.hipGetDevice(C.byref(device)) == 0
    assert ask(C.byref(count), _ATTRIBUTE_MULTIPROCESSOR_COUNT, device.value) == 0
    assert 0 < count.value <= 4096, count.value
    return count.value


# ---------------------------------------------------------------------------------------
# inputs and reference, once per process
# ---------------------------------------------------------------------------------------
_references = {}


def reference(shape, offset=0.0):
    """``filter_support.reference`` computed once per process; nobody writes to what it returns."""
    key = (shape, offset)
    if key not in _references:
        out = fs.reference(shape, offset)
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _references[key] = out
    return _references[key]


def blurred_pairs(x, y, params, L_ref):
    """pairs whose reference depends on its own float64 templates by more than a tenth of RTOL_L (filter_support.
    reference_resolution): none may be, then the comparison of the chain with L_ref needs no allowance"""
    return fs.reference_resolution(x, y, params) > 0.1 * fs.RTOL_L * np.abs(L_ref).astype(np.float64)


def own_lines(shape):
    """(A, mu, sig) [ndata] of the lines ``filter_support.make_inputs`` put into the spectra of ``shape`` (A = 0: none):
    its random sequence replayed (test_chunk_shapes_host.py rebuilds the spectra from these and compares)."""
    ndata, _, nx, B = shape
    rng = np.random.RandomState(1000 * nx + 7 * ndata + B)
    x = np.linspace(400, 800, nx) if nx > 200 else np.linspace(400, 800, 200)[:nx]
    lo, hi = x[0] - 2.0, x[-1] + 2.0
    noise = rng.normal(0, fs.NOISE, size=(nx, ndata))
    lined = rng.uniform(size=ndata) < 0.8
    A = np.where(lined, 0.02 / rng.power(3, size=ndata), 0.0)
    mu, sig = rng.uniform(lo, hi, size=ndata), 10 ** rng.uniform(0.3, 1.3, size=ndata)
    return A, mu, sig, noise


def lone_winner(shape, c, params, rows):
    """Candidates with number ``c`` made the own line of the strongest-lined spectrum ``d`` of the selection: under
    thresholds nobody beats but for one ulp below ``L[c, d]`` at ``d``, candidate ``c`` alone is accepted -- provided it
    is the strict maximum of column ``d``, which the caller asserts on the values it decides with.  -> d, params"""
    A, mu, sig, _ = own_lines(shape)
    sel = np.arange(shape[0]) if rows is None else rows
    d = int(sel[np.argmax(A[sel])])
    out = np.array(params)
    out[c] = (A[d], mu[d], sig[d])
    return d, np.ascontiguousarray(out)


def lone_candidates(B):
    """the last candidate of a chunk, and the first one of its last tile of four where that is another"""
    return sorted(set((B - 1, 4 * ((B - 1) // 4))), reverse=True)


def strict_margin(L, c, d):
    """by how much (relative) L[c, d] lies above every other candidate's value for data set d; +inf alone"""
    others = np.delete(L[:, d], c)
    return np.inf if len(others) == 0 else float((L[c, d] - others.max()) / np.abs(L[c, d]))


def backend_state(spectra, nlive, shelf_cap=64):
    """A Gaussian-line joint state whose draws go through the backend entry points, initialised -- the backend scores
    with the noise level ``mdns_joint_init_gauss`` was given -- with ``nlive`` points that ``mdns_joint_set_live`` then
    replaces."""
    from massivedatans_amd import jointstate
    js = jointstate.GaussJointState(spectra, nlive, lambda p: p, shelf_cap=shelf_cap, fetch_rows=False, via_backend=True)
    js.init(np.tile(np.array([[0.1, 500.0, 10.0]]), (nlive, 1)))
    return js


def planted_live(thr):
    live = np.full((NLIVE, len(thr)), FILLER)
    live[0] = thr
    return np.ascontiguousarray(live)


def tie_places(M):
    """positions of the selection whose thresholds the tie cases plant: tile and wave edges and the last one"""
    return sorted(set(p for p in (0, 15, 16, 63, 64, M - 1) if p < M))


def check_outcome(got, thr, rows, L, Lall):
    """The outcome ``(index, fill bits, thresholds afterwards, shelf sizes afterwards)`` of ONE chunk on a planted state
    (thresholds ``thr``, empty shelves) against the decision ``L`` [B, ndata] gives: the index, the fill bits position
    by position, one point waiting where it beats, and the thresholds afterwards -- with one point waiting the second
    smallest of {thr, the point, the fillers}: the point -- bit for bit ``Lall[idx, d]``, the chain's value, and
    untouched elsewhere, outside the selection in particular."""
    idx, beats, after, n1 = got
    want_idx, want_beats = fs.decision(L, thr, rows)
    assert idx == want_idx, (idx, want_idx)
    sel = np.arange(len(thr)) if rows is None else rows
    want_thr, want_n = thr.copy(), np.zeros(len(thr), dtype=int)
    if idx >= 0:
        assert beats is not None and np.array_equal(beats, want_beats), np.flatnonzero(beats != want_beats)
        want_thr[sel[want_beats]] = Lall[idx, sel[want_beats]]
        want_n[sel[want_beats]] = 1
    else:
        assert beats is None
    assert np.array_equal(n1, want_n), np.flatnonzero(n1 != want_n)
    assert np.array_equal(after, want_thr), np.flatnonzero(after != want_thr)


# ---------------------------------------------------------------------------------------
# the statement of a draw of several chunks
# ---------------------------------------------------------------------------------------
def threshold(col, shelf):
    """the (len(shelf) + 1)-th smallest of live + shelf, NaN being no value; +inf when there are fewer"""
    values = np.concatenate((col, shelf))
    values = np.sort(values[~np.isnan(values)])
    return values[len(shelf)] if len(shelf) < len(values) else np.inf


class Statement(object):
    """Live points and shelves in numpy.  A chunk is decided on the likelihoods it is GIVEN, [B, ndata] over all data
    sets -- the chain's own values: thresholds become earlier candidates' likelihoods, so ties are real and compare
    strictly.  The first candidate that beats the threshold of some selected data set goes onto the shelves of the
    selected data sets it beats, and their thresholds are recomputed from the two arrays."""

    def __init__(self, live):
        self.live = np.array(live, dtype=np.float64)
        self.nlive, self.ndata = self.live.shape
        self.shelf = [np.zeros(0) for _ in range(self.ndata)]
        self.higher = np.full(self.ndata, np.nan)

    def sizes(self):
        return np.array([len(s) for s in self.shelf])

    def prepare(self):
        for d in range(self.ndata):
            col = self.live[:, d]
            real = col[~np.isnan(col)]
            m = real.min() if len(real) else np.inf
            self.shelf[d] = self.shelf[d][self.shelf[d] > m]
            self.higher[d] = threshold(col, self.shelf[d])

    def votes(self, L, rows):
        """one 0 / 1 vote per candidate: some selected data set accepts it"""
        sel = np.arange(self.ndata) if rows is None else np.asarray(rows)
        with np.errstate(invalid="ignore"):
            return (L[:, sel] > self.higher[sel]).any(axis=1).astype(np.int32)

    def commit(self, L, rows, idx):
        """candidate ``idx`` is taken in by the selected data sets it beats -> which (bool over the selection)"""
        sel = np.arange(self.ndata) if rows is None else np.asarray(rows)
        with np.errstate(invalid="ignore"):
            beats = L[idx, sel] > self.higher[sel]
        for d in sel[beats]:
            self.shelf[d] = np.append(self.shelf[d], L[idx, d])
            self.higher[d] = threshold(self.live[:, d], self.shelf[d])
        return beats

    def chunk(self, L, rows):
        """-> (accepted index or -1, who it beats over the selection or None)"""
        v = self.votes(L, rows)
        if not v.any():
            return -1, None
        idx = int(np.argmax(v))
        return idx, self.commit(L, rows, idx)


def pack_bits(bits):
    """bool [n] -> uint64 [ceil(n / 64)], bit k of word k / 64 = bits[k], the rest zero"""
    bits = np.asarray(bits, dtype=bool)
    padded = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


class RawDraws(object):
    """A Gaussian-line joint state driven through the raw entry points a native constrainer calls: one
    ``mdns_backend_draw_begin`` per draw, then any number of ``mdns_backend_draw_chunk``."""

    def __init__(self, spectra, live, shelf_cap=64):
        from massivedatans_amd import _lib
        self._lib_module = _lib
        self.js = backend_state(spectra, len(live), shelf_cap=shelf_cap)
        self.lib, self.h = self.js._lib, self.js._h
        self.ndata = self.js.ndata
        live = np.ascontiguousarray(live, dtype=np.float64)
        _lib.check(self.lib.mdns_joint_set_live(self.h, _lib.ptr(live)), "mdns_joint_set_live")
        self.js.prepare()
        self._rows, self._M = None, self.ndata

    def close(self):
        self.js.close()

    def begin(self, rows):
        self._rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        self._M = self.ndata if rows is None else len(rows)
        self._lib_module.check(self.lib.mdns_backend_draw_begin(self.h, self._lib_module.opt(self._rows), self._M), "mdns_backend_draw_begin")

    def chunk(self, params):
        """-> accepted index, fill words (None when nobody was accepted), nscored, the kernel that scored the chunk"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        accepted, nscored = C.c_int(-2), C.c_int(-2)
        words = np.zeros((self._M + 63) // 64, dtype=np.uint64)
        ptr = self._lib_module.ptr
        self._lib_module.check(self.lib.mdns_backend_draw_chunk(self.h, ptr(params), len(params), None, C.addressof(accepted), ptr(words),
                                                                C.addressof(nscored)), "mdns_backend_draw_chunk")
        name = (self.lib.mdns_profile_kernel(0) or b"").decode()
        return accepted.value, (words if accepted.value >= 0 else None), nscored.value, name

    def cap(self):
        return self.lib.mdns_joint_shelf_cap(self.h)

    def thresholds(self):
        return self.js.thresholds()


def compare_chunk(driver, ref, params, L, rows, route, what):
    """One chunk on the statement and -- unless ``driver`` is None -- on the device: accepted index, fill words,
    nscored, thresholds and shelf sizes afterwards and the kernel name, all exactly.  -> the statement's (index, beats)"""
    idx, beats = ref.chunk(L, rows)
    if driver is not None:
        got, words, nscored, name = driver.chunk(params)
        assert got == idx, (what, "accepted", got, idx)
        if idx >= 0:
            assert np.array_equal(words, pack_bits(beats)), (what, "fill words")
        assert nscored == len(params), (what, "nscored", nscored)
        higher, n = driver.thresholds()
        assert np.array_equal(n, ref.sizes()), (what, "shelf sizes", np.flatnonzero(n != ref.sizes()))
        assert np.array_equal(higher, ref.higher), (what, "thresholds", np.flatnonzero(higher != ref.higher))
        check_route(name, route)
    return idx, beats


def lines(rng, B, x, faint=1.0):
    """B candidates (A, mu, sig): A log-uniform in [0.01, 1] times ``faint``, mu over the grid, sig log-uniform in [1, 100]"""
    return np.ascontiguousarray(np.column_stack([faint * 10 ** rng.uniform(-2, 0, size=B), rng.uniform(x[0] - 2.0, x[-1] + 2.0, size=B),
                                                 10 ** rng.uniform(0, 2, size=B)]))


def reference_scorer(x, y):
    """``score(params) -> L [B, ndata]`` from the plain statement, in float64: what the host file runs the sequences on"""
    return lambda params: fs.reference_loglike(x, y, params).astype(np.float64)


# ---------------------------------------------------------------------------------------
# the sequences.  ``score(params) -> L [B, ndata]``; ``make_driver(live, shelf_cap) -> RawDraws or None``; ``num_cus``
# for the expected routes.  Each returns what happened, for the caller to print; what must happen is asserted on the
# statement, so the host file shows it with no device.
# ---------------------------------------------------------------------------------------
SEQUENCE_A_SHAPE = (200, "2/3", 208, 9)
SEQUENCE_A_CAP = 4
SEQUENCE_A_NLIVE = 3


def sequence_a(score, make_driver, num_cus):
    """Rows from the mapped block, then from the device; repeats that tie with the shelves; the shelves growing inside
    the draw."""
    shape = SEQUENCE_A_SHAPE
    x, y, params, rows = fs.make_inputs(shape)
    M, nx = len(rows), shape[2]
    rng = np.random.RandomState(208)
    live = score(lines(rng, SEQUENCE_A_NLIVE, x))
    ref = Statement(live)
    ref.prepare()
    driver = make_driver(live, SEQUENCE_A_CAP)
    try:
        if driver is not None:
            driver.begin(rows)
            assert driver.cap() == SEQUENCE_A_CAP
        Lall = score(params)
        log = []
        for n, (a, b) in enumerate(((0, 1), (1, 4), (4, 9), (0, 9), (0, 9))):
            route = expected_route(M, b - a, nx, num_cus)
            if n >= 3:
                # a repeat: whoever was accepted before now lies ON the thresholds it set
                assert (Lall[a:b][:, rows] == ref.higher[rows]).any(), "the repeat ties with nothing"
            idx, beats = compare_chunk(driver, ref, params[a:b], Lall[a:b], rows, route, ("a", n))
            log.append((b - a, route, idx))
        assert any(idx >= 0 for _, _, idx in log[:3]), "no candidate of the shape was accepted"
        # fresh faint lines: six chunks at the least, and until some shelf of the selection holds more than the state
        # was made for -- the accept kernel reads the rows it left on the device while the shelves move to a larger block
        for n in range(40):
            if n >= 6 and (ref.sizes()[rows] > SEQUENCE_A_CAP).any():
                break
            B = (9, 5, 2)[n % 3]
            fresh = lines(rng, B, x, faint=(0.3, 0.3, 0.05, 0.1)[n % 4])
            route = expected_route(M, B, nx, num_cus)
            idx, beats = compare_chunk(driver, ref, fresh, score(fresh), rows, route, ("a", "fresh", n))
            log.append((B, route, idx))
        assert (ref.sizes()[rows] > SEQUENCE_A_CAP).any(), "no shelf of the selection passed %d entries" % SEQUENCE_A_CAP
        outside = np.setdiff1d(np.arange(shape[0]), rows)
        assert not ref.sizes()[outside].any()
        if driver is not None:
            assert driver.cap() > SEQUENCE_A_CAP, "the shelves did not grow"
        return log
    finally:
        if driver is not None:
            driver.close()


SEQUENCE_B_NDATA, SEQUENCE_B_NX = 4200, 8


def sequence_b_inputs():
    x, y, _, _ = fs.make_inputs((SEQUENCE_B_NDATA, None, SEQUENCE_B_NX, 26))
    rows = np.setdiff1d(np.arange(SEQUENCE_B_NDATA), np.arange(0, SEQUENCE_B_NDATA, 41)).astype(np.int32)
    assert len(rows) == 4097
    return x, y, rows


def sequence_b(score, make_driver, num_cus):
    """A route switch inside a draw over more than 4096 spectra: chunks of 8 (two-launch, rows from the mapped block), 9
    (classic, on the rows the first kernel left) and 4 candidates (two-launch, from the device copy); a second draw in
    the order 9, 8, 9, where the classic chunk uploads the rows first."""
    x, y, rows = sequence_b_inputs()
    M, nx = len(rows), SEQUENCE_B_NX
    rng = np.random.RandomState(4200)
    live = score(lines(rng, 6, x))
    ref = Statement(live)
    ref.prepare()
    driver = make_driver(live, 64)
    try:
        log = []
        for draw, sizes in enumerate(((8, 9, 4), (9, 8, 9))):
            if driver is not None:
                driver.begin(rows)
            for n, B in enumerate(sizes):
                fresh = lines(rng, B, x, faint=(1.0, 0.3, 0.1)[n])
                route = expected_route(M, B, nx, num_cus)
                idx, beats = compare_chunk(driver, ref, fresh, score(fresh), rows, route, ("b", draw, n))
                log.append((B, route, idx))
        # every chunk accepts somebody: each one's thresholds are those the chunk before it -- of the other route -- left
        assert all(idx >= 0 for _, _, idx in log), log
        outside = np.setdiff1d(np.arange(SEQUENCE_B_NDATA), rows)
        assert not ref.sizes()[outside].any()
        return log
    finally:
        if driver is not None:
            driver.close()


SEQUENCE_C_NDATA, SEQUENCE_C_NX = 300, 64


def sequence_c(score, make_driver, num_cus):
    """Both commit kernels behind one another on one state: draws over selections of 128, 129 and 64 spectra in turn
    (k_chunk_commit, k_joint_commit_trail, k_chunk_commit), two chunks each."""
    x, y, _, _ = fs.make_inputs((SEQUENCE_C_NDATA, None, SEQUENCE_C_NX, 16))
    rng = np.random.RandomState(300)
    live = score(lines(rng, 6, x))
    ref = Statement(live)
    ref.prepare()
    driver = make_driver(live, 64)
    try:
        log = []
        for M in (128, 129, 64):
            rows = np.sort(rng.choice(SEQUENCE_C_NDATA, size=M, replace=False)).astype(np.int32)
            if driver is not None:
                driver.begin(rows)
            for n, B in enumerate((5, 3)):
                fresh = lines(rng, B, x, faint=(1.0, 0.1)[n])
                route = expected_route(M, B, SEQUENCE_C_NX, num_cus)
                idx, beats = compare_chunk(driver, ref, fresh, score(fresh), rows, route, ("c", M, n))
                log.append((M, B, route, idx))
        assert all(idx >= 0 for _, _, _, idx in log), log
        return log
    finally:
        if driver is not None:
            driver.close()


# ---------------------------------------------------------------------------------------
# the halves
# ---------------------------------------------------------------------------------------
def halves_plan(shape, L, thr, rows):
    """What the halves must do at ``shape`` under thresholds ``thr`` when the likelihoods are ``L`` [B, ndata]: the
    steps of test_chunk_shapes.py::test_halves on the statement alone.  -> the statement at the end and, step by step,
    (votes, who to clear or vote for, the index the commit accepts, who it beats)."""
    ref = Statement(planted_live(thr))
    ref.prepare()
    steps = []
    # 1. the first vote cleared: the second voted candidate is taken in
    votes = ref.votes(L, rows)
    assert votes.sum() >= 2, "fewer than two candidates have votes"
    first, second = (int(b) for b in np.flatnonzero(votes)[:2])
    cleared = votes.copy()
    cleared[first] = 0
    beats = ref.commit(L, rows, second)
    assert beats.any()
    steps.append((votes, cleared, second, beats))
    # 2. a single foreign vote, on a candidate nobody accepts: accepted with no bit set
    votes = ref.votes(L, rows)
    free = np.flatnonzero(votes == 0)
    assert len(free), "every candidate is accepted by somebody"
    foreign = np.zeros(len(votes), dtype=np.int32)
    foreign[free[len(free) // 2]] = 1
    steps.append((votes, foreign, int(np.argmax(foreign)), np.zeros(len(beats), dtype=bool)))
    # 3. the honest commit
    idx, beats = ref.chunk(L, rows)
    steps.append((votes, votes, idx, beats))
    return ref, steps
