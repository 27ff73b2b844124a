"""The cases test_k2_filter_shapes.py runs under every configuration of the K2 matrix-core filter
(csrc/mdns_k2gemm.hip), each configuration in a child pytest process over this file (the library reads
MDNS_K2_FILTER_* once per process; k2_filter_support.child_environment).  Not collected with the suite: the file
name keeps it out, and outside such a child every case fails at once.

Part A runs the pass alone (mdns_muse_filter_dev) over k2_filter_support.SHAPES and holds its votes, marks and count
to the plain statement in np.longdouble; Part B does the same through the joint state (mdns_backend_draw_band);
Part C walks shapes small, large, small in one process and repeats a launch with split tiles a hundred times."""
import hashlib
import os
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate
from massivedatans_amd.like import MuseSpectra
import k2_filter_support as ks

sys.path.insert(0, os.path.join(ks.ROOT, "tools"))
import k2_filter_bench as kb  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIG = os.environ.get(ks.CONFIG_VARIABLE)
FILLER = 1e300          # live points nobody looks at: above every likelihood


@pytest.fixture(autouse=True)
def _in_a_child():
    assert CONFIG in ks.CONFIGS, "these cases run in a child of test_k2_filter_shapes.py (%s names the configuration)" % ks.CONFIG_VARIABLE
    for k, v in ks.child_environment(CONFIG).items():
        if k.startswith("MDNS_K2_FILTER"):
            assert os.environ.get(k) == v, (k, os.environ.get(k), v)
    assert not [k for k in os.environ if k.startswith("MDNS_K2_FILTER") and k not in ks.CONFIGS[CONFIG]]


def _kernel(hip):
    return (hip.mdns_profile_kernel(1) or b"").decode()


class _Pass(object):
    """The spectra of a case on the device, plain and with the NaN channel, its templates, and the buffers of
    mdns_muse_filter_dev; ``run`` is one launch."""

    def __init__(self, hip, case):
        self.hip, self.case = hip, case
        self.spectra = {False: MuseSpectra(case.x, case.y, case.v), True: MuseSpectra(case.x, case.y_nan, case.v)}
        self.flags = np.zeros(2 * case.B + 1, dtype=np.int32)
        self.d_t = self._up(case.templates)
        self.d_rows = self._up(case.rows) if case.rows is not None else None
        self.d_thr, self.d_bound, self.d_flags = (hip.mdns_dev_alloc(n) for n in (8 * case.ndata, 8 * case.B, self.flags.nbytes))
        self.want_kernel = ks.expected_kernel(CONFIG, case.ndata, case.nx, case.B, case.rows, case.M)

    def _up(self, a):
        a = np.ascontiguousarray(a)
        d = self.hip.mdns_dev_alloc(a.nbytes)
        assert d
        _lib.check(self.hip.mdns_h2d(d, _lib.ptr(a), a.nbytes), "h2d")
        return d

    def run(self, with_nan, bound, thr):
        hip, case = self.hip, self.case
        zero = np.zeros_like(self.flags)
        thr, bound = np.ascontiguousarray(thr), np.ascontiguousarray(bound)
        assert thr.shape == (case.ndata,) and bound.shape == (case.B,)
        for d, a in ((self.d_thr, thr), (self.d_bound, bound), (self.d_flags, zero)):
            _lib.check(hip.mdns_h2d(d, _lib.ptr(a), a.nbytes), "h2d")
        _lib.check(hip.mdns_muse_filter_dev(self.spectra[with_nan].handle, self.d_t, case.B, self.d_rows, case.M, self.d_thr,
                                            self.d_bound, self.d_flags), "mdns_muse_filter_dev")
        _lib.check(hip.mdns_d2h(_lib.ptr(self.flags), self.d_flags, self.flags.nbytes), "d2h")
        assert _kernel(hip) == self.want_kernel, ("another instantiation scored the pass", _kernel(hip), self.want_kernel)
        B = case.B
        return self.flags[:B].copy(), self.flags[B:2 * B].copy(), int(self.flags[2 * B])

    def run_and_check(self, launch):
        with_nan, bound, thr = launch
        clear, maybe, count = self.run(with_nan, bound, thr)
        self.case.check(clear, maybe, count, self.case.classify(with_nan, bound, thr))

    def close(self):
        for d in (self.d_t, self.d_rows, self.d_thr, self.d_bound, self.d_flags):
            if d:
                self.hip.mdns_dev_free(d)
        for s in self.spectra.values():
            s.close()


# ---------------------------------------------------------------------------------------
# Part A: the pass alone
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ks.SHAPES, ids=ks.shape_id)
def test_pass_alone(hip, shape):
    """Every launch of a shape (k2_filter_support.Case.launches: the all-zero bound over spectra with a NaN channel,
    the graded bound over the plain ones, four threshold draws each) against the statement's demands."""
    case = ks.Case(shape)
    assert ks.preconditions(case)[0] == 0
    p = _Pass(hip, case)
    for launch in case.launches():
        p.run_and_check(launch)
    p.close()


# ---------------------------------------------------------------------------------------
# Part B: the same through the joint state
# ---------------------------------------------------------------------------------------
SHAPES_B = [(33, 40, 17, None, 0), (250, 700, 65, "third", 0), (100, 257, 57, None, 0)]
NLIVE = 3
#: offsets that keep a pair outside the band whatever the slack: no 0 and no +-0.5
OUTSIDE = np.array([-1.5, 1.5, -10.0, 10.0, -1e6, 1e6])


def _device_reference(case, templates):
    """(A, Lq) of the statement for the templates the DEVICE made of the case's parameters, shared between the
    children by the templates' bytes."""
    cache = os.environ.get(ks.CACHE_VARIABLE)
    path = os.path.join(cache, "B-%s-%s.npz" % (ks.shape_id(case.shape), hashlib.sha1(templates.tobytes()).hexdigest())) if cache else None
    if path and os.path.exists(path):
        with np.load(path) as f:
            return f["A"], f["Lq"]
    A, Lq = ks.reference_filter(case.y, case.v, templates)
    if path:
        tmp = path + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, A=A, Lq=Lq)
        os.replace(tmp, path)
    return A, Lq


def _state(spectra, case, thr):
    st = jointstate.MuseJointState(spectra, NLIVE, shelf_cap=4)
    st.init(case.params[np.arange(NLIVE) % case.B])
    live = np.full((NLIVE, case.ndata), FILLER)
    live[0] = thr
    st._check(st._lib.mdns_joint_set_live(st._h, _lib.ptr(np.ascontiguousarray(live))), "mdns_joint_set_live")
    st.prepare()
    before, n0 = st.thresholds()
    assert np.array_equal(before, thr) and not n0.any()
    return st


@pytest.mark.parametrize("shape", SHAPES_B, ids=ks.shape_id)
def test_through_the_joint_state(hip, shape):
    """mdns_backend_draw_band with mdns_muse_filter_mode(1).  First with every pair outside band + S: the statuses
    are the statement's, the chunk was filtered and not scored again, and after the commit of the first clear
    candidate the fill bits, thresholds (rtol 1e-10, the project's bar for K2) and shelf counts are those Lq gives.
    Then with one pair planted on its threshold: the chunk is handed to the exact kernels, and the listed pairs are
    exactly the statement's."""
    case = ks.Case(shape)
    ndata, B, M, sel = case.ndata, case.B, case.M, case.sel
    spectra = MuseSpectra(case.x, case.y, case.v)
    templates = spectra.templates(case.params)
    assert np.allclose(templates, case.templates, rtol=1e-12, atol=0)
    A, Lq = _device_reference(case, templates)
    case._ref = (A, Lq)                                            # (classify and thresholds speak of the device's templates)
    bound = np.zeros(B)
    # thresholds that keep every pair of the selection outside band + S: the first draw that does
    for k in range(40):
        offsets = OUTSIDE[np.random.RandomState(case.draw_seed + 100 + k).randint(len(OUTSIDE), size=ndata)]
        play = sel[[(M - 1) // 5 + k % 2, M // 2, (4 * M) // 5]]
        offsets[play] = [-1.5, 1.5, -10.0]
        thr = case.thresholds(A, Lq, bound, offsets)
        thr[thr == -1e300] = Lq[np.arange(ndata) % B, np.arange(ndata)][thr == -1e300].astype(np.float64)   # (the state's: any)
        # (all but three data sets of the selection nobody beats: else nearly every candidate votes clear)
        top = Lq.max(axis=0)
        nobody = np.ones(ndata, dtype=bool)
        nobody[play] = False
        thr[nobody] = (top + 10 * (np.longdouble(2e-12) * np.abs(top) + np.longdouble(case.gamma) * A))[nobody].astype(np.float64)
        want = case.classify(False, bound, thr)
        if want["listed"] == 0 and want["slivers"] == 0 and want["clear_must"].any() and not want["clear_must"].all():
            break
    else:
        raise AssertionError("no draw of thresholds keeps every pair outside its band")
    try:
        st = _state(spectra, case, thr)
        s0 = kb.stats(hip)
        res = kb.band(st, case.params, case.rows, bound, 1)
        assert _kernel(hip) == ks.expected_kernel(CONFIG, ndata, case.nx, B, case.rows, M), _kernel(hip)
        s1 = kb.stats(hip)
        assert np.array_equal(res[0], want["clear_must"].astype(np.int32)), np.flatnonzero(res[0] != want["clear_must"])
        assert res[1] == 0
        assert [b - a for a, b in zip(s0, s1)][:3] == [1, 0, 0]            # filtered, not scored again
        first = int(np.flatnonzero(want["clear_must"])[0])
        bits = np.zeros((M + 63) // 64, dtype=np.uint64)
        st._check(hip.mdns_backend_draw_band_commit(st._h, first, _lib.ptr(np.zeros(M)), _lib.ptr(bits)), "draw_band_commit")
        s2 = kb.stats(hip)
        assert [b - a for a, b in zip(s1, s2)][:3] == [0, 0, 1]            # the exact row of the accepted candidate
        beats = want["must_clear"][first]
        got = (bits[np.arange(M) // 64] >> (np.arange(M) % 64).astype(np.uint64)) & np.uint64(1)
        assert np.array_equal(got.astype(bool), beats), np.flatnonzero(got.astype(bool) != beats)
        after, n1 = st.thresholds()
        want_n = np.zeros(ndata, dtype=int)
        want_n[sel[beats]] = 1
        want_thr = thr.copy()
        want_thr[sel[beats]] = Lq[first, sel[beats]].astype(np.float64)     # (the point is the second smallest of thr, it, the fillers)
        assert np.array_equal(n1, want_n)
        assert np.allclose(after, want_thr, rtol=1e-10, atol=0)
        untouched = np.ones(ndata, dtype=bool)
        untouched[sel[beats]] = False
        assert np.array_equal(after[untouched], thr[untouched])
        st.close()
        # one pair planted on its threshold
        d0 = int(sel[M // 3])
        k0 = int(np.flatnonzero(sel == d0)[0])
        thr2 = thr.copy()
        thr2[d0] = np.float64(Lq[d0 % B, d0])
        want2 = case.classify(False, bound, thr2)
        assert want2["slivers"] == 0 and want2["listed"] == 1 and want2["must_list"][d0 % B, k0]
        st = _state(spectra, case, thr2)
        s0 = kb.stats(hip)
        res = kb.band(st, case.params, case.rows, bound, 1)
        s1 = kb.stats(hip)
        assert [b - a for a, b in zip(s0, s1)][:2] == [1, 1]               # filtered, then handed to the exact kernels
        assert res[1] == 1 and list(res[2]) == [d0 % B] and list(res[3]) == [k0], res[1:4]
        status = np.where(want2["clear_must"], 1, np.where(want2["maybe_must"], 2, 0))
        assert np.array_equal(res[0], status), np.flatnonzero(res[0] != status)
        st.close()
    finally:
        hip.mdns_muse_filter_mode(-1)
        spectra.close()


# ---------------------------------------------------------------------------------------
# Part C: state across launches
# ---------------------------------------------------------------------------------------
def test_state_across_launches(hip):
    """Shapes small, large, small in ONE process: the scratch of the hand-over, the delivery counts and the tiled
    template buffer grow and are reused (stale columns past B); every launch checked as in Part A.  Under the
    configurations with the busiest hand-over, then a hundred launches of 250 x 700 x 65 -- its tiles split over
    workgroups --, fresh thresholds every tenth, every output checked (each launch also shows that the one before
    left the delivery counts at zero), and last a case whose tiles split differently."""
    passes = {}
    for at in ks.ORDER_C:
        case = ks.Case(ks.SHAPES[at])
        p = passes[at] = _Pass(hip, case)
        for launch in case.launches():
            p.run_and_check(launch)
    if CONFIG in ks.REPEAT_CONFIGS:
        p = passes[ks.REPEAT_SHAPE]
        case = p.case
        fresh = [launch for launch in case.launches(draws=ks.REPEATS // 10, first_draw=3) if not launch[0]]
        assert len(fresh) == ks.REPEATS // 10
        wants = [case.classify(*launch) for launch in fresh]
        for rep in range(ks.REPEATS):
            launch, want = fresh[rep // 10], wants[rep // 10]
            clear, maybe, count = p.run(*launch)
            case.check(clear, maybe, count, want)
        other = _Pass(hip, ks.Case(ks.SHAPES[11]))
        for launch in other.case.launches(draws=1):
            other.run_and_check(launch)
        other.close()
    for p in passes.values():
        p.close()
