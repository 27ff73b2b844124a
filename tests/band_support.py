"""The band form of the likelihood noise (include/mdns.h Part 5: mdns_backend_draw_band, its _begin / _ready / _end
halves and _commit) on planted thresholds: test_band_planted.py on the device, test_band_host.py without one.

Here, in plain numpy: the float64 statement of one chunk's decisions (:func:`statement`), the solver that puts a threshold
EXACTLY on an edge of the band (:func:`edge_thresholds`), the case generators (a case is a list of rounds, every round one
threshold vector and one bound vector for the same likelihood block), the classes a case must contain, the ``(npairs,
cap)`` table of ``_end`` and the planting on a device state.

What is exact.  The device computes ``band = 1.01 * bound[b] + 1e-12 * (|L| + |thr|)`` and compares ``L > thr + band`` and
``L >= thr - band``.  With ``bound[b] = 0`` the first product is an exact zero, so the band is one rounded sum times one
constant whether or not the compiler contracts the expression into an fma: the float64 statement is then bit for bit what
the device decides, and a threshold can be planted on an edge.  With ``bound[b] > 0`` a contraction may move the band by
an ulp: such pairs are planted at graded distances and every one of them must be UNAMBIGUOUS -- the same class with the
band scaled by ``1 - 2**-50``, ``1`` and ``1 + 2**-50`` (:func:`ambiguous`; none is allowed)."""
import numpy as np

#: kinds of the exact-edge rounds (bound = 0), by where the threshold sits relative to the chosen candidate's likelihood
EDGE_KINDS = ("upper-edge", "below-upper-edge", "lower-edge", "above-lower-edge", "equal", "far-below", "far-above", "+inf", "-inf")
#: what the statement must say of the planted pair of each kind
EDGE_CLASS = {"upper-edge": "listed", "below-upper-edge": "clear", "lower-edge": "listed", "above-lower-edge": "silent",
              "equal": "listed", "far-below": "clear", "far-above": "silent"}
#: L - thr in units of the band, in the graded rounds (bound > 0 for most candidates)
GRADED_OFFSETS = (0.0, 0.5, -0.5, 1 - 1e-6, -(1 - 1e-6), 1 + 1e-6, -(1 + 1e-6), 1.5, -1.5, 10.0, -10.0, 1e6, -1e6)
GRADED_KINDS = tuple("off%+g" % o for o in GRADED_OFFSETS) + ("+inf", "-inf")
BOUNDS = (4e-5, 0.0, 1e-9)
#: the classes every case must show (test_band_host.py asserts them on the statement; the device tests lean on that)
REQUIRED = ("upper-edge", "below-upper-edge", "lower-edge", "above-lower-edge", "status0", "status1", "status2", "clear-with-pairs")
SCAN_ULPS = 240
K_BAND_CAP = 4096                      # csrc/mdns_internal.h kBandCap: pairs of a chunk the device keeps


# ---------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------
def band_of(L, thr, bound, scale=1.0):
    with np.errstate(invalid="ignore", over="ignore"):
        return (1.01 * np.asarray(bound)[:, None] + 1e-12 * (np.abs(L) + np.abs(thr)[None, :])) * scale


def classes(L, thr, bound, scale=1.0, nonfinite_rule=True):
    """-> clear [B, M], inside [B, M].  ``nonfinite_rule``: the band of a likelihood that is not finite is 0 (the rule
    of constrainer.python_backend)."""
    L, thr = np.asarray(L, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    band = band_of(L, thr, bound, scale)
    if nonfinite_rule:
        band[~np.isfinite(L)] = 0.0
    with np.errstate(invalid="ignore"):
        clear = L > thr[None, :] + band
        inside = ~clear & (L >= thr[None, :] - band)
    return clear, inside


def statement(L, thr, bound, nonfinite_rule=True):
    """One chunk: ``status`` int [B] (1 some pair clear, else 2 some pair inside, else 0), the pairs inside the band
    sorted by (b, k) -- ``pair_b``, ``pair_k``, ``pair_L``, ``pair_thr`` -- and ``npairs``."""
    L, thr = np.asarray(L, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    clear, inside = classes(L, thr, bound, 1.0, nonfinite_rule)
    status = np.where(clear.any(axis=1), 1, np.where(inside.any(axis=1), 2, 0)).astype(np.int32)
    b, k = np.nonzero(inside)                              # row-major: sorted by (b, k)
    return {"status": status, "npairs": len(b), "pair_b": b.astype(np.int32), "pair_k": k.astype(np.int32),
            "pair_L": L[b, k], "pair_thr": thr[k], "clear": clear, "inside": inside}


def ambiguous(L, thr, bound):
    """bool [B, M]: pairs with ``bound[b] != 0`` whose class changes with the band scaled by 1 -+ 2**-50 (what a
    contraction of the band's expression can do and more).  Pairs with ``bound[b] == 0`` are exact: never ambiguous."""
    base = classes(L, thr, bound)
    out = np.zeros(np.shape(L), dtype=bool)
    for scale in (1.0 - 2.0 ** -50, 1.0 + 2.0 ** -50):
        c, i = classes(L, thr, bound, scale)
        out |= (c != base[0]) | (i != base[1])
    out[np.asarray(bound) == 0.0, :] = False
    return out


def end_table(n, cap):
    """What ``mdns_backend_draw_band_end`` hands over when ``n`` pairs were inside the band and the caller's arrays hold
    ``cap`` entries -> (entries copied, the ``*npairs`` returned).  With ``room = min(cap, 4096)``: n <= room: all n and
    n itself; n > room: ``room`` entries and a number above ``cap`` (n, or cap + 1 where n <= cap): the caller falls back."""
    room = min(cap, K_BAND_CAP)
    if n <= room:
        return n, n
    return room, (cap + 1 if n <= cap else n)


# ---------------------------------------------------------------------------------------
# thresholds exactly on an edge (bound = 0)
# ---------------------------------------------------------------------------------------
def _band0(v, thr):
    return 1e-12 * (np.abs(v) + np.abs(thr))


def _scan(centre):
    """the doubles within SCAN_ULPS of ``centre``, ascending"""
    i = np.array(centre, dtype=np.float64).reshape(1).view(np.int64)[0]
    c = (i + np.arange(-SCAN_ULPS, SCAN_ULPS + 1, dtype=np.int64)).view(np.float64)
    return np.sort(c)


def edge_thresholds(v):
    """For a finite ``v != 0`` and ``bound = 0``: ``(upper, lower)``.  ``upper`` is the SMALLEST double thr with
    ``thr + band == v`` (on it the pair is listed, one ulp of thr below it the pair is clear), ``lower`` the LARGEST with
    ``thr - band == v`` (listed; one ulp above: silent).  None where the scan of +-240 ulps finds no exact solution or the
    neighbour is not of the other class."""
    v = float(v)
    c = _scan(v - 2e-12 * abs(v))
    hit = c[c + _band0(v, c) == v]
    upper = None
    if len(hit):
        t, below = hit[0], np.nextafter(hit[0], -np.inf)
        if v > below + _band0(v, below):
            upper = float(t)
    c = _scan(v + 2e-12 * abs(v))
    hit = c[c - _band0(v, c) == v]
    lower = None
    if len(hit):
        t, above = hit[-1], np.nextafter(hit[-1], np.inf)
        if not v >= above - _band0(v, above):
            lower = float(t)
    return upper, lower


# ---------------------------------------------------------------------------------------
# the cases: rounds of (thr [M], bound [B]) for one block L [B, M]
# ---------------------------------------------------------------------------------------
def _far(v):
    return 0.01 * abs(v) + 1.0


def _edge_threshold(kind, v, misses):
    if kind in ("upper-edge", "below-upper-edge", "lower-edge", "above-lower-edge"):
        upper, lower = edge_thresholds(v)
        t = upper if "upper" in kind else lower
        if t is None:
            misses.append((kind, v))
            return v
        if kind == "below-upper-edge":
            return float(np.nextafter(t, -np.inf))
        if kind == "above-lower-edge":
            return float(np.nextafter(t, np.inf))
        return t
    return {"equal": v, "far-below": v - _far(v), "far-above": v + _far(v), "+inf": np.inf, "-inf": -np.inf}[kind]


def _graded_threshold(off, b, d, L, bound):
    """thr with ``L[b, d] - thr = off`` bands (the band taken at the threshold found).  An offset a millionth of a band
    from an edge is moved outwards, by factors of 4, until the pair is unambiguous: at |L| = 1e7 a millionth of the band of
    a small bound is less than an ulp of L."""
    v = L[b, d]
    near = abs(abs(off) - 1.0) < 0.01
    dev = abs(abs(off) - 1.0)
    while True:
        o = np.sign(off) * (1.0 + np.sign(abs(off) - 1.0) * dev) if near else off
        thr = v - o * (1.01 * bound[b] + 2e-12 * abs(v))
        thr = v - o * (1.01 * bound[b] + 1e-12 * (abs(v) + abs(thr)))
        if not near or dev >= 0.25 or not ambiguous(L[b:b + 1, d:d + 1], np.array([thr]), bound[b:b + 1])[0, 0]:
            return float(thr)
        dev *= 4.0


def nrounds(B, M, nkinds):
    return int(min(max(1, -(-nkinds * B // M)), 3 * nkinds))


def edge_rounds(L):
    """Exact-edge rounds, ``bound = 0``: with ``i = d + round * M`` the threshold of data set ``d`` sits relative to
    candidate ``i % B`` as kind ``(i // B) % 9`` says; as many rounds as it takes every candidate to meet every kind (27
    at most), then one round with every threshold above every candidate (status 0) and one with every threshold on an
    edge of, or equal to, the best candidate of its data set (status 2, nobody clear).
    -> (rounds, misses of the solver); a round is a dict of thr, bound, who [M], kind [M], name."""
    B, M = L.shape
    nk = len(EDGE_KINDS)
    rounds, misses = [], []
    for r in range(nrounds(B, M, nk)):
        i = np.arange(M) + r * M
        who, kind = i % B, (i // B) % nk
        thr = np.array([_edge_threshold(EDGE_KINDS[kind[d]], L[who[d], d], misses) for d in range(M)])
        rounds.append({"thr": thr, "bound": np.zeros(B), "who": who, "kind": [EDGE_KINDS[k] for k in kind], "name": "edge%d" % r})
    best = np.argmax(L, axis=0)
    top = L[best, np.arange(M)]
    kinds = [("far-above", "+inf")[d % 2] for d in range(M)]
    rounds.append({"thr": np.array([_edge_threshold(kinds[d], top[d], misses) for d in range(M)]), "bound": np.zeros(B), "who": best,
                   "kind": kinds, "name": "edge-nobody"})
    kinds = [("upper-edge", "lower-edge", "equal")[d % 3] for d in range(M)]
    rounds.append({"thr": np.array([_edge_threshold(kinds[d], top[d], misses) for d in range(M)]), "bound": np.zeros(B), "who": best,
                   "kind": kinds, "name": "edge-listed-only"})
    return rounds, misses


def graded_rounds(L):
    """Graded rounds: ``bound[b] = BOUNDS[(b + round) % 3]`` (one of them 0), thresholds at GRADED_OFFSETS bands from the
    chosen candidate's likelihood, and +-inf; then the two rounds for status 0 and status 2 as in :func:`edge_rounds`
    (half a band inside instead of on the edge)."""
    B, M = L.shape
    nk = len(GRADED_KINDS)
    rounds = []
    for r in range(max(nrounds(B, M, nk), 3 if B < 3 else 1)):       # (fewer than three candidates: three rounds, every bound occurs)
        bound = np.array([BOUNDS[(b + r) % 3] for b in range(B)])
        i = np.arange(M) + r * M
        who, kind = i % B, (i // B) % nk
        thr = np.empty(M)
        for d in range(M):
            name = GRADED_KINDS[kind[d]]
            thr[d] = {"+inf": np.inf, "-inf": -np.inf}[name] if name in ("+inf", "-inf") else \
                _graded_threshold(GRADED_OFFSETS[kind[d]], who[d], d, L, bound)
        rounds.append({"thr": thr, "bound": bound, "who": who, "kind": [GRADED_KINDS[k] for k in kind], "name": "graded%d" % r})
    bound = np.array([BOUNDS[b % 3] for b in range(B)])
    best = np.argmax(L + 1.01 * bound[:, None], axis=0)
    top = L[best, np.arange(M)]
    far = top + 1.01 * bound[best] + np.array([_far(t) for t in top]) + 10 * bound.max()
    rounds.append({"thr": np.where(np.arange(M) % 2 == 0, far, np.inf), "bound": bound, "who": best,
                   "kind": ["far-above" if d % 2 == 0 else "+inf" for d in range(M)], "name": "graded-nobody"})
    # half a band around the highest lower edge (L - band): its owner is inside, nobody is clear
    edge = L - band_of(L, top, bound)
    best = np.argmax(edge, axis=0)
    thr = np.array([_graded_threshold((0.5, -0.5, 0.0)[d % 3], best[d], d, L, bound) for d in range(M)])
    rounds.append({"thr": thr, "bound": bound, "who": best, "kind": ["off%+g" % (0.5, -0.5, 0.0)[d % 3] for d in range(M)],
                   "name": "graded-listed-only"})
    return rounds


def seen_classes(L, rounds):
    """names of REQUIRED (and every kind planted) that the statement finds over the rounds of a case; the planted pair of
    an exact-edge kind must be of the class EDGE_CLASS says"""
    seen = set()
    for rd in rounds:
        st = statement(L, rd["thr"], rd["bound"])
        for d, (b, kind) in enumerate(zip(rd["who"], rd["kind"])):
            cls = "clear" if st["clear"][b, d] else "listed" if st["inside"][b, d] else "silent"
            if kind in EDGE_CLASS and (rd["bound"][b] == 0.0) and np.isfinite(L[b, d]):
                assert cls == EDGE_CLASS[kind], (rd["name"], d, b, kind, cls)
            seen.add(kind)
        seen |= {"status%d" % s for s in st["status"]}
        if ((st["status"] == 1) & st["inside"].any(axis=1)).any():
            seen.add("clear-with-pairs")
    return seen


def synthetic_L(B, M, seed):
    """negative likelihoods, |L| from 1e1 to 1e7, no two candidates of a data set close"""
    rng = np.random.RandomState(seed)
    mag = 10 ** rng.uniform(1, 7, size=M)
    return -(mag[None, :] * (1.0 + rng.permutation(B)[:, None] + rng.uniform(0.0, 0.5, size=(B, M))))


# ---------------------------------------------------------------------------------------
# planting on the device
# ---------------------------------------------------------------------------------------
def live_for(thr, nlive):
    """a live matrix whose row 0 is ``thr`` and whose other rows lie far above it"""
    thr = np.asarray(thr, dtype=np.float64)
    finite = np.where(np.isfinite(thr), thr, 0.0)
    live = np.abs(finite)[None, :] + 1e6 * (1.0 + np.arange(nlive))[:, None]
    live[:, thr == np.inf] = np.inf
    live[0] = thr
    return np.ascontiguousarray(live)


def plant(st, thr):
    """``thr`` [ndata] becomes the threshold of every data set of the device state ``st`` (shelves emptied)"""
    from massivedatans_amd import _lib
    live = live_for(thr, st.nlive)
    st._check(st._lib.mdns_joint_set_live(st._h, _lib.ptr(live)), "mdns_joint_set_live")
    st.shelf_n[:] = 0
    st.set_running(np.arange(st.ndata))
    st.prepare()
    got = st.thresholds()[0]
    assert np.array_equal(got, thr), "the planted thresholds are not the state's"
    return live


def full_thresholds(thr_sel, rows, ndata, rest=np.inf):
    """thresholds of a selection spread over all data sets (the others: ``rest``)"""
    if rows is None:
        return np.asarray(thr_sel, dtype=np.float64)
    out = np.full(ndata, rest, dtype=np.float64)
    out[np.asarray(rows)] = thr_sel
    return out
