"""The exact routes of the band form of the likelihood noise (mdns_backend_draw_band, its _begin / _ready / _end halves and
_commit) on planted thresholds, against the float64 statement of tests/band_support.py -- exactly: the likelihoods are the
device's own (``loglike_batch_lines`` with the same candidates, selection and handle gives the bits the band scores with,
test_k2_rows.py::test_a_pair_has_one_value), the thresholds are planted through the live matrix, and with ``bound = 0`` the
statement is bit for bit what the device computes.

Two routes make the decisions: the vote that rides along in ``k_muse_rows<NP, 2>`` (small chunks: pairs of candidates per
workgroup, no continuum, nx <= 4096), and ``k_joint_band`` behind a dense scoring (everything else).  After every band call
``mdns_profile_kernel(1)`` must name the kernel the case was built for.  The matrix-core filter stays out (mode 0).

A selection of ``mdns_backend_draw_begin`` is ascending by contract (a scrambled one is refused: asserted here), so the
selections below are ascending ones with gaps."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from massivedatans_amd import _lib
import band_support as bs
import joint_planted_support as jps
import k2_rows_support as ks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import k2_filter_bench as kb  # noqa: E402

NLIVE = 6
GUARD = 64
SENTINEL_I, SENTINEL_F = -77, -7.7e77


@pytest.fixture(scope="module")
def num_cus():
    """(asked in a child process, as in test_k2_rows.py: torch's own HIP runtime finds no device behind the library's)"""
    import subprocess
    code = "import torch; print(int(torch.cuda.get_device_properties(0).multi_processor_count))"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module", autouse=True)
def exact_routes_only():
    lib = _lib.require_device()
    lib.mdns_muse_filter_mode(0)
    try:
        yield
    finally:
        lib.mdns_muse_filter_mode(-1)


def launched():
    return (_lib.load().mdns_profile_kernel(1) or b"").decode()


def expected_kernel(route, nx, B, M, num_cus, continuum):
    """the scoring kernel of a band chunk, and that it belongs to the route the case was built for"""
    if continuum:
        assert route == "dense"
        return "k_continuum_rows<"
    name = ks.expected_kernel(nx, B, M, num_cus)
    fused = name.startswith("k_muse_rows<") and name.endswith(", 2>")
    assert fused == (route == "fused"), (route, name)
    return name


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def selection(ndata, M):
    """M of ndata data sets, ascending, with gaps, the last one among them (None: all)"""
    if M == ndata:
        return None
    rows = np.sort(np.random.RandomState(ndata).choice(ndata - 1, size=M - 1, replace=False)) if M > 1 else np.zeros(0, dtype=int)
    return np.concatenate((rows, [ndata - 1])).astype(np.int32)


def make_state(ndata, nx, B, seed, continuum=0):
    """spectra, state and B candidates whose lines are hundreds of channels wide: at nx = 8 (one channel every 657 A) the
    lines of the prior fall between the channels and every candidate would have the same flat template -- and the same
    likelihoods, so that a mixed-up candidate index would go unseen"""
    sp, st, _, _, _ = kb.planted_state(ndata, nx, NLIVE, B, seed, [0.0], continuum=continuum)
    assert st._lib.mdns_joint_shelf_cap(st._h) == 4
    rng = np.random.RandomState(seed + 1)
    params = np.column_stack((rng.uniform(-1.0, 1.0, B), rng.uniform(0.0, 0.02, B), rng.uniform(2.2, 2.8, B),
                              rng.uniform(0.2, 2.0, B), rng.uniform(0.2, 2.0, B)))
    return sp, st, np.ascontiguousarray(params)


def distinct(L):
    """no two candidates share a likelihood on any data set"""
    s = np.sort(L, axis=0)
    return bool((s[1:] != s[:-1]).all())


def same_as_statement(got, L, thr, bound, what):
    """status, npairs and the pair list sorted by (b, k) of one band call (as kb.band returns them) against the statement"""
    want = bs.statement(L, thr, bound)
    status, npairs, pb, pk, pL, pthr = got[:6]
    assert np.array_equal(status, want["status"]), (what, status, want["status"])
    assert npairs == want["npairs"], (what, npairs, want["npairs"])
    assert np.array_equal(pb, want["pair_b"]) and np.array_equal(pk, want["pair_k"]), what
    assert np.array_equal(bits(pL), bits(want["pair_L"])), what
    assert np.array_equal(bits(pthr), bits(want["pair_thr"])), what
    return want


def run_rounds(st, params, rows, L, rounds, kernel, what):
    thr_of = {}
    for rd in rounds:
        bs.plant(st, bs.full_thresholds(rd["thr"], rows, st.ndata))
        got = kb.band(st, params, rows, rd["bound"], 0)
        assert launched().startswith(kernel) and (kernel.endswith("<") or launched() == kernel), (what, rd["name"], launched(), kernel)
        same_as_statement(got, L, rd["thr"], rd["bound"], (what, rd["name"]))
        thr_of[rd["name"]] = rd["thr"]
    return thr_of


# ------------------------------------------------------------------ (A) decisions and pair lists on planted thresholds
def _cases(n):
    many = 2 * n
    return [
        # the vote in k_muse_rows<NP, 2>
        ("fused", 2, 1, 8, 0), ("fused", 3, 1, 8, 0), ("fused", 2, 64, 8, 0), ("fused", 3, 130, 8, 0),
        ("fused", 33, 70, 8, 0),                     # candidates split over grid.y, odd tail
        ("fused", 2, 8 * n + 37, 8, 0),              # rows looped inside a workgroup
        ("fused", 3, many + 5, 8, 0),                # B < 4 stays fused at any M
        ("fused", 5, many - 1, 8, 0),                # one spectrum under the two-row switch
        ("fused", 3, 5, 513, 0), ("fused", 2, 7, 4096, 0), ("fused", 5, 9, 700, 0),
        # k_joint_band behind a dense scoring
        ("dense", 1, 1, 8, 0), ("dense", 1, 257, 8, 0),                       # k_muse_rows<NP, 1>; two workgroups in x
        ("dense", 5, many, 8, 0), ("dense", 9, many + 300, 8, 0),            # two-row kernel; several x B workgroups publish
        ("dense", 3, 40, 4097, 0), ("dense", 2, 5, 4610, 0),                  # past the fused kernel's channels: the generic one
        ("dense", 4, 70, 8, 1),                                               # continuum
    ]


NCASES = len(_cases(256))


@pytest.mark.parametrize("selected", (False, True), ids=("all", "selected"))
@pytest.mark.parametrize("index", range(NCASES))
def test_decisions_on_planted_thresholds(index, selected, num_cus):
    route, B, M, nx, continuum = _cases(num_cus)[index]
    ndata = M + 5 if selected else M
    rows = selection(ndata, M)
    sp, st, params = make_state(ndata, nx, B, 1000 + index, continuum)
    try:
        kernel = expected_kernel(route, nx, B, M, num_cus, continuum)
        L = sp.loglike_batch_lines(params, rows)
        assert launched().startswith(kernel), (launched(), kernel)
        assert L.shape == (B, M) and np.isfinite(L).all() and (L != 0).all() and distinct(L)
        edge, misses = bs.edge_rounds(L)
        assert misses == []
        graded = bs.graded_rounds(L)
        assert sum(int(bs.ambiguous(L, rd["thr"], rd["bound"]).sum()) for rd in graded) == 0
        seen = bs.seen_classes(L, edge)
        if M >= len(bs.EDGE_KINDS) * B:
            assert seen >= set(bs.EDGE_KINDS) | {"status0", "status1", "status2"}
        t0 = time.perf_counter()
        run_rounds(st, params, rows, L, edge + graded, kernel, (route, B, M, nx))
        print("%s B=%d M=%d nx=%d %s: %d rounds, %.3f s on the device" % (route, B, M, nx, "selected" if selected else "all", len(edge) + len(graded),
                                                                           time.perf_counter() - t0))
    finally:
        st.close()
        sp.close()


def test_a_scrambled_selection_is_refused():
    sp, st, params = make_state(9, 8, 2, 5)
    try:
        rows = np.array([2, 0, 5], dtype=np.int32)
        assert st._lib.mdns_backend_draw_begin(st._h, _lib.ptr(rows), 3) != 0
        assert "ascending" in _lib.last_error()
    finally:
        st.close()
        sp.close()


# ------------------------------------------------------------------ (B) overflow of the pair list, reuse of the scratch
def raw_band(st, params, rows, bound, cap, halves):
    """One band call into arrays of exactly ``cap`` entries followed by a guard -> status, *npairs, the four arrays whole.
    ``halves``: through _begin / _ready / _end, _ready polled (a bounded number of times) until it says 1."""
    lib = st._lib
    B = len(params)
    M = st.ndata if rows is None else len(rows)
    st._check(lib.mdns_backend_draw_begin(st._h, _lib.ptr(rows) if rows is not None else None, M), "draw_begin")
    status, npairs = np.full(B, SENTINEL_I, dtype=np.int32), C.c_int(SENTINEL_I)
    pb, pk = np.full(cap + GUARD, SENTINEL_I, dtype=np.int32), np.full(cap + GUARD, SENTINEL_I, dtype=np.int32)
    pL, pthr = np.full(cap + GUARD, SENTINEL_F), np.full(cap + GUARD, SENTINEL_F)
    p, bound = np.ascontiguousarray(params), np.ascontiguousarray(bound)
    out = (_lib.ptr(status), C.byref(npairs), _lib.ptr(pb), _lib.ptr(pk), _lib.ptr(pL), _lib.ptr(pthr), cap)
    if halves:
        st._check(lib.mdns_backend_draw_band_begin(st._h, _lib.ptr(p), B, _lib.ptr(bound)), "draw_band_begin")
        for _ in range(5000):
            if lib.mdns_backend_draw_band_ready(st._h) == 1:
                break
            time.sleep(0.001)
        assert lib.mdns_backend_draw_band_ready(st._h) == 1, "the chunk's outcome did not arrive within 5000 polls"
        st._check(lib.mdns_backend_draw_band_end(st._h, *out), "draw_band_end")
    else:
        st._check(lib.mdns_backend_draw_band(st._h, _lib.ptr(p), B, _lib.ptr(bound), *out), "draw_band")
    return status, npairs.value, pb, pk, pL, pthr


def check_overflow(got, L, thr, bound, cap, what):
    """the table of ``_end``; what was copied are genuine pairs of the statement, each once; nothing else was written"""
    want = bs.statement(L, thr, bound)
    status, npairs, pb, pk, pL, pthr = got
    copied, reported = bs.end_table(want["npairs"], cap)
    assert np.array_equal(status, want["status"]), what
    assert npairs == reported, (what, npairs, reported, want["npairs"])
    for a, s in ((pb, SENTINEL_I), (pk, SENTINEL_I), (pL, SENTINEL_F), (pthr, SENTINEL_F)):
        assert (a[copied:] == s).all(), (what, "written behind the %d entries handed over" % copied)
    b, k = pb[:copied], pk[:copied]
    assert ((b >= 0) & (b < L.shape[0]) & (k >= 0) & (k < L.shape[1])).all(), what
    assert want["inside"][b, k].all(), (what, "a pair that is not inside its band")
    assert len(set(zip(b.tolist(), k.tolist()))) == copied, (what, "a pair listed twice")
    assert np.array_equal(bits(pL[:copied]), bits(L[b, k])) and np.array_equal(bits(pthr[:copied]), bits(thr[k])), what
    if copied == want["npairs"]:
        order = np.lexsort((k, b))
        assert np.array_equal(b[order], want["pair_b"]) and np.array_equal(k[order], want["pair_k"]), what
    return want


@pytest.fixture(scope="module")
def big(num_cus):
    ndata = max(600, 2 * num_cus + 88)
    sp, st, params = make_state(ndata, 8, 9, 77)
    L = sp.loglike_batch_lines(params, None)
    assert np.isfinite(L).all() and distinct(L)
    yield {"sp": sp, "st": st, "params": params, "ndata": ndata, "L": L}
    st.close()
    sp.close()


def _exactly(L, target):
    """thresholds and bounds with exactly ``target`` pairs inside: six candidates whose bound swallows everything, one
    whose threshold is its own likelihood on the first data sets, the thresholds of the rest above everybody"""
    B, M = L.shape
    bound = np.array([1e300] * 6 + [0.0] * (B - 6))
    n = target - 6 * M
    assert 0 < n < M
    for _ in range(8):
        thr = np.where(np.arange(M) < n, L[6], L.max(axis=0) + 0.01 * np.abs(L).max(axis=0) + 1.0)
        have = bs.statement(L, thr, bound)["npairs"]
        if have == target:
            return thr, bound
        n += target - have
    raise AssertionError("no threshold vector with exactly %d pairs inside" % target)


@pytest.mark.parametrize("halves", (False, True), ids=("one-call", "begin-ready-end"))
def test_overflow_and_reuse_of_the_scratch(big, halves, num_cus):
    """More pairs inside the band than the device keeps (4096) and than the caller has room for, at ``cap`` below, at and
    above 4096 -- ``cap = 5000`` is the case whose copy used to run past the device's box --; exactly 4096 and 4097 pairs;
    and right behind them a small chunk that must find counter, ticket and votes reset."""
    st, params, L, ndata = big["st"], big["params"], big["L"], big["ndata"]
    B = len(params)
    kernel = expected_kernel("dense", 8, B, ndata, num_cus, 0)
    assert kernel == "k_muse_rows2<1>"
    thr = L[0].copy()
    bs.plant(st, thr)
    everything = np.full(B, 1e300)
    assert bs.statement(L, thr, everything)["npairs"] == B * ndata > 5000
    for cap in (64, 4096, 5000):
        got = raw_band(st, params, None, everything, cap, halves)
        assert launched() == kernel
        check_overflow(got, L, thr, everything, cap, ("all inside", cap))
    for target in (4096, 4097):
        thr, bound = _exactly(L, target)
        bs.plant(st, thr)
        for cap in (4096, 5000):
            got = raw_band(st, params, None, bound, cap, halves)
            assert launched() == kernel
            want = check_overflow(got, L, thr, bound, cap, (target, cap))
            assert want["npairs"] == target
    # 3 x 40 on the same handle, thresholds 1 % away from the candidate they are made of, no bound: nothing is listed
    rows = np.arange(40, dtype=np.int32)
    L3 = big["sp"].loglike_batch_lines(params[:3], rows)
    assert launched() == expected_kernel("fused", 8, 3, 40, num_cus, 0)
    own = L3[np.arange(40) % 3, np.arange(40)]
    thr3 = own + np.where(np.arange(40) % 2 == 0, 0.01, -0.01) * np.abs(own)
    want = bs.statement(L3, thr3, np.zeros(3))
    assert want["npairs"] == 0
    bs.plant(st, bs.full_thresholds(thr3, rows, ndata))
    got = raw_band(st, params[:3], rows, np.zeros(3), 4096, halves)
    assert launched() == expected_kernel("fused", 8, 3, 40, num_cus, 0)
    assert np.array_equal(got[0], want["status"]) and got[1] == 0
    assert (got[2] == SENTINEL_I).all() and (got[4] == SENTINEL_F).all()
    # ... and all nine against thresholds above everybody: no vote of the large chunks is left with candidates 3 to 8
    L9 = big["sp"].loglike_batch_lines(params, rows)
    high = L9.max(axis=0) + 0.01 * np.abs(L9).max(axis=0)
    bs.plant(st, bs.full_thresholds(high, rows, ndata))
    got = raw_band(st, params, rows, np.zeros(B), 4096, halves)
    assert np.array_equal(got[0], np.zeros(B, dtype=np.int32)) and got[1] == 0


# ------------------------------------------------------------------ (C) non-finite values
@pytest.mark.parametrize("slot", (0, 1), ids=("even-slot", "odd-slot"))
def test_a_nan_candidate_beside_a_sound_one(slot, num_cus):
    """A candidate with a NaN parameter in either place of a fused pair: status 0 and no pair for it; its partner's status
    and pairs as in the run without it."""
    sp, st, params = make_state(40, 8, 2, 31)
    try:
        kernel = expected_kernel("fused", 8, 2, 40, num_cus, 0)
        L = sp.loglike_batch_lines(params, None)
        assert np.isfinite(L).all() and distinct(L)
        edge, misses = bs.edge_rounds(L)
        assert misses == []
        bad = params.copy()
        bad[slot, 0] = np.nan
        Lbad = sp.loglike_batch_lines(bad, None)
        print("NaN parameter: likelihoods", Lbad[slot, :4])
        assert np.isnan(Lbad[slot]).all() and np.array_equal(bits(Lbad[1 - slot]), bits(L[1 - slot]))
        for rd in edge + bs.graded_rounds(L):
            bs.plant(st, rd["thr"])
            clean = kb.band(st, params, None, rd["bound"], 0)
            same_as_statement(clean, L, rd["thr"], rd["bound"], rd["name"])
            got = kb.band(st, bad, None, rd["bound"], 0)
            assert launched() == kernel
            same_as_statement(got, Lbad, rd["thr"], rd["bound"], rd["name"])
            assert got[0][slot] == 0 and not (got[2] == slot).any()
            assert got[0][1 - slot] == clean[0][1 - slot]
            mine, theirs = got[2] == 1 - slot, clean[2] == 1 - slot
            for a, b in zip(got[2:6], clean[2:6]):
                assert np.array_equal(a[mine], b[theirs])
    finally:
        st.close()
        sp.close()


def test_an_amplitude_of_1e200(num_cus):
    """log amplitude 200: whatever the scoring returns for it, the band treats it as the statement with the rule of
    constrainer.python_backend does (a likelihood that is not finite has no band)."""
    sp, st, params = make_state(40, 8, 3, 32)
    try:
        L = sp.loglike_batch_lines(params, None)
        assert np.isfinite(L).all() and distinct(L)
        edge, misses = bs.edge_rounds(L)
        assert misses == []
        huge = params.copy()
        huge[1, 0] = 200.0
        Lh = sp.loglike_batch_lines(huge, None)
        print("log_amp = 200: likelihoods", Lh[1, :6], "finite:", int(np.isfinite(Lh[1]).sum()), "nan:", int(np.isnan(Lh[1]).sum()),
              "-inf:", int((Lh[1] == -np.inf).sum()), "+inf:", int((Lh[1] == np.inf).sum()))
        assert np.array_equal(bits(Lh[[0, 2]]), bits(L[[0, 2]]))
        for rd in edge + bs.graded_rounds(L):
            bs.plant(st, rd["thr"])
            got = kb.band(st, huge, None, rd["bound"], 0)
            assert launched() == expected_kernel("fused", 8, 3, 40, num_cus, 0)
            same_as_statement(got, Lh, rd["thr"], rd["bound"], rd["name"])
    finally:
        st.close()
        sp.close()


# ------------------------------------------------------------------ (D) the commit on planted noise rows
class BandDriver(jps.DeviceDriver):
    """joint_planted_support's driver over a MUSE state that is already there"""

    def __init__(self, st):
        self._lib_module = _lib
        self.js, self.lib, self.h = st, st._lib, st._h
        self.nlive, self.ndata = st.nlive, st.ndata

    def close(self):
        pass


def _landing(v, target):
    """j with v + j == target exactly, or None"""
    j0 = target - v
    for j in (j0, np.nextafter(j0, np.inf), np.nextafter(j0, -np.inf)):
        if v + j == target:
            return j
    return None


def noise_row(Lb, thr, turn):
    """jitter [M]: per data set the sum L + j lands exactly on the threshold (not beaten), one ulp above it (beaten), far
    on either side, or j = 0 -- and j = 0 wherever L == thr or the threshold is not finite"""
    M = len(Lb)
    row = np.zeros(M)
    for k in range(M):
        v, t = Lb[k], thr[k]
        if not np.isfinite(t) or v == t:
            continue
        kind = 2 if k % 7 == 0 else (k + turn) % 5         # (one data set in seven is beaten every time: its shelf grows)
        j = None
        if kind == 0:
            j = _landing(v, t)
        elif kind == 1:
            j = _landing(v, np.nextafter(t, np.inf))
        elif kind == 2:
            j = (t - v) + 3.0 * (turn + 1) + 0.001 * abs(t)
        elif kind == 3:
            j = (t - v) - 3.0 - 0.001 * abs(t)
        row[k] = 0.0 if j is None else j
    return row


def commit_and_compare(st, ref, rows, L, b, turn, what):
    sel = np.arange(st.ndata) if rows is None else rows
    M = len(sel)
    row = noise_row(L[b], ref.higher[sel], turn)
    nwords = (M + 63) // 64
    words = np.full(nwords + 2, np.uint64(0xdeadbeefdeadbeef), dtype=np.uint64)
    st._check(st._lib.mdns_backend_draw_band_commit(st._h, b, _lib.ptr(row), _lib.ptr(words)), "mdns_backend_draw_band_commit")
    idx, beats = ref.chunk((L[b] + row)[None, :], rows)
    if beats is None:
        beats = np.zeros(M, dtype=bool)
    assert np.array_equal(words[:nwords], jps.pack_bits(beats)), (what, "fill words")
    assert (words[nwords:] == np.uint64(0xdeadbeefdeadbeef)).all()
    st.took(rows, beats)
    higher, n = st.thresholds()
    assert np.array_equal(n, ref.sizes()), (what, "shelf sizes")
    assert np.array_equal(bits(higher), bits(ref.higher)), (what, "thresholds")
    return beats


def start_reference(st, live):
    ref = jps.Reference(st.nlive, st.ndata)
    ref.live = live.copy()
    ref.prepare()
    return ref


@pytest.mark.parametrize("route,B,Mof", (("fused", 3, lambda n: 130), ("dense", 9, lambda n: 2 * n + 300)), ids=("fused-3x130", "dense-9xmany"))
def test_commit_on_planted_noise_rows(route, B, Mof, num_cus):
    """After a band call the host names the accepted candidate and hands its noise row over: fill words, thresholds and
    shelf sizes of ALL data sets (a sparse selection), and the committed values read back in order, against the brute-force
    reference of joint_planted_support fed with L[b] + row.  First a candidate that is accepted only through a listed pair;
    then five commits of clear candidates onto the same data sets, the shelves (4 entries at first) growing under them."""
    M = Mof(num_cus)
    ndata = M + 9
    rows = selection(ndata, M)
    sp, st, params = make_state(ndata, 8, B, 400 + B)
    try:
        kernel = expected_kernel(route, 8, B, M, num_cus, 0)
        L = sp.loglike_batch_lines(params, rows)
        assert np.isfinite(L).all() and distinct(L)
        edge, misses = bs.edge_rounds(L)
        assert misses == []
        by_name = {rd["name"]: rd for rd in edge}
        driver = BandDriver(st)
        zero = np.zeros(B)
        # accepted through a listed pair alone
        rd = by_name["edge-listed-only"]
        ref = start_reference(st, bs.plant(st, bs.full_thresholds(rd["thr"], rows, ndata)))
        want = same_as_statement(kb.band(st, params, rows, zero, 0), L, rd["thr"], zero, "listed only")
        assert launched() == kernel and not (want["status"] == 1).any()
        b = int(np.flatnonzero(want["status"] == 2)[0])
        beats = commit_and_compare(st, ref, rows, L, b, 1, "listed only")
        assert beats.any() and want["inside"][b][beats].any() and {"on-threshold", "one-ulp"} <= ref.seen
        assert jps.read_out(driver, ref) >= 1
        # clear candidates, five times
        rd = by_name["edge0"]
        ref = start_reference(st, bs.plant(st, bs.full_thresholds(rd["thr"], rows, ndata)))
        assert st._lib.mdns_joint_shelf_cap(st._h) == 4
        for turn in range(5):
            thr = ref.higher[rows]
            want = same_as_statement(kb.band(st, params, rows, zero, 0), L, thr, zero, ("turn", turn))
            assert launched() == kernel
            clear = np.flatnonzero(want["status"] == 1)
            assert len(clear)
            b = int(clear[turn % len(clear)])
            beats = commit_and_compare(st, ref, rows, L, b, turn, ("turn", turn))
            assert beats.any() and not beats.all()
        assert {"on-threshold", "one-ulp"} <= ref.seen
        assert ref.sizes().max() == 5 and st._lib.mdns_joint_shelf_cap(st._h) > 4
        sel = np.zeros(ndata, dtype=bool)
        sel[rows] = True
        assert (ref.sizes()[~sel] == 0).all()
        assert jps.read_out(driver, ref) == 5
    finally:
        st.close()
        sp.close()
