"""The chained first batch of a fresh region (csrc/mdns_chain.hip behind mdns_backend_chain_begin /
_chain_end: box proposals, membership counts, keep test, rank compaction, prior transform with the
double-double 10**v, templates, accept test, commit -- without a host look in between) against its numpy
statement ``constrainer.chain_statement``, driven through the entry points by ctypes, no sampler.

Everything is compared exactly.  Counts, kept proposals and chunk size are integers; the parameters the
device scored with must be, bit for bit, the statement's with ``pow10_dd`` of the same header built for
the host (the same IEEE operations in the same order: a difference is a contraction or a table error);
accept decision and fill bits must be those of ``jointstate.HostJointState`` fed by the lane kernel with
the DEVICE's parameters.  Membership counts come three ways: the chain's, K3 of the product on the
statement's proposals (a second region with the radius set) and the CPU oracle's.

The module runs once in a child process with a short MDNS_POLL_TIMEOUT_S (the library reads it once per
process), so that a lost mailbox fails a case in seconds; the tests of the parent report the child's
outcome case by case.  After a polled wait that timed out the child starts nothing more on the device."""
import ctypes as C
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from massivedatans_amd import _lib, constrainer, jointstate, sample
from massivedatans_amd.clustering import neighbors
from massivedatans_amd.like import GaussLineSpectra
from chain_support import LaneScorer, make_request, pow10_dd  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_CHILD = os.environ.get("MDNS_CHAIN_TESTS_CHILD") == "1"
NBOOT = 15


@pytest.fixture(scope="module")
def child_report(tmp_path_factory):
    """Outcome of every case of this module, run once in a child with a short poll timeout."""
    xml = str(tmp_path_factory.mktemp("chain") / "report.xml")
    env = dict(os.environ, MDNS_CHAIN_TESTS_CHILD="1", MDNS_POLL_TIMEOUT_S="15")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu", "--junitxml=" + xml,
                          os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1100)
    cases = {}
    if os.path.exists(xml):
        for tc in ET.parse(xml).getroot().iter("testcase"):
            bad = [c for c in tc if c.tag in ("failure", "error", "skipped")]
            cases[tc.get("name")] = "\n".join((c.get("message") or "") + "\n" + (c.text or "") for c in bad) if bad else None
    print(out.stdout[-6000:])
    return cases, out


@pytest.fixture
def child(request):
    """``child()`` is False in the child process (the case runs); in the parent it asserts that the child
    passed this very case and returns True."""
    if IN_CHILD:
        return lambda: False
    cases, out = request.getfixturevalue("child_report")
    name = request.node.name

    def reported():
        assert name in cases, "the child process did not run %s (exit %d):\n%s" % (name, out.returncode, out.stdout[-3000:] + out.stderr[-2000:])
        assert cases[name] is None, cases[name][-6000:]
        return True
    return reported


def call(rc, what):
    """A library call that must succeed; a polled wait that timed out ends the child."""
    if rc != 0:
        msg = _lib.last_error()
        if "MDNS_POLL_TIMEOUT_S" in msg:
            pytest.exit("%s: %s -- nothing more is started on the device" % (what, msg), returncode=3)
        raise AssertionError("%s failed: %s" % (what, msg))


_fn = {}


def entry(name):
    """mdns_backend_chain_begin / _end with the prototypes of the backend table."""
    if name not in _fn:
        _fn[name] = C.cast(getattr(_lib.require_device(), "mdns_backend_" + name),
                           constrainer._CHAIN_BEGIN if name == "chain_begin" else constrainer._CHAIN_END)
    return _fn[name]


_spectra = {}


def spectra_for(nx, ndata):
    """``ndata`` spectra of ``nx`` channels: noise and one line each, at different places."""
    if (nx, ndata) not in _spectra:
        rng = np.random.RandomState(nx * 131 + ndata)
        x = np.linspace(400.0, 800.0, nx)
        centre, height = rng.uniform(420, 780, size=ndata), 0.02 / rng.power(3, size=ndata)
        y = height[None, :] * np.exp(-0.5 * ((centre[None, :] - x[:, None]) / 8.0) ** 2) + rng.normal(0, 0.01, size=(nx, ndata))
        _spectra[(nx, ndata)] = GaussLineSpectra(x, np.ascontiguousarray(y), noise_level=0.01)
    return _spectra[(nx, ndata)]


def prior_of(ndim, kind="sample"):
    """``sample``: sample.py's prior on the first three dimensions (A = 10**(2u - 2), mu = 400u + 400,
    sig = 10**(2u)), further dimensions the identity; ``b0``: no offsets anywhere; ``plain``: no power at all;
    ``twice``: ``pow10`` and ``kernel_pow10`` on the same dimension."""
    p = constrainer.Prior()
    p.ndim, p.nparams = ndim, 3
    rows = {"sample": ((2.0, -2.0, 1, 0), (400.0, 400.0, 0, 0), (2.0, 0.0, 0, 1)),
            "b0": ((-2.0, 0.0, 1, 0), (800.0, 0.0, 0, 0), (2.0, 0.0, 0, 1)),
            "plain": ((0.05, 0.001, 0, 0), (400.0, 400.0, 0, 0), (90.0, 2.0, 0, 0)),
            "twice": ((2.0, -2.0, 1, 0), (400.0, 400.0, 0, 0), (0.3, 0.0, 1, 1)),
            # (lines about as high and as wide as the spectra's own, anywhere on the grid: which candidate fits a
            # spectrum best depends on the spectrum)
            "lines": ((0.02, 0.015, 0, 0), (400.0, 400.0, 0, 0), (0.2, 0.8, 0, 1))}[kind]
    for k in range(ndim):
        p.a[k], p.b[k], p.pow10[k], p.kernel_pow10[k] = rows[k] if k < 3 else (1.0, 0.0, 0, 0)
    return p


def ulps_apart(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


class Setup(object):
    """One region (members, bootstrap choice), one batch of raw doubles, one joint state on the device
    and its numpy statement beside it."""

    def __init__(self, ndim=3, n=1000, K=200, nx=200, ndata=100, nlive=20, seed=0, spread=0.15, joint="gauss"):
        assert joint in ("gauss", "muse")
        self.rng = rng = np.random.RandomState(seed * 1000 + ndim * 100 + n + K)
        self.ndim, self.n, self.K, self.ndata = ndim, n, K, ndata
        self.members = np.ascontiguousarray(0.5 + spread * rng.uniform(-1, 1, size=(K, ndim)))
        idx = rng.randint(0, K, size=(NBOOT, K))
        self.masks = np.zeros(K, dtype=np.uint32)
        for b in range(NBOOT):
            hit = np.zeros(K, dtype=np.uint32)
            hit[idx[b]] = 1 << b
            self.masks |= hit
        self.u = np.ascontiguousarray(rng.uniform(size=(n, ndim)))
        self.mn, self.mx = self.members.min(axis=0), self.members.max(axis=0)
        # the radius K6 gives, from the synchronous entry point; the region keeps serving K3 for the statement
        self.ms, self.radius = neighbors.MemberSet.bootstrapped(self.members, self.masks, NBOOT)
        self.lib = _lib.require_device()
        if joint == "gauss":
            self.spectra = spectra_for(nx, ndata)
            self.dev = jointstate.GaussJointState(self.spectra, nlive, sample.kernel_params, fetch_rows=False, via_backend=True)
            self.host = jointstate.HostJointState(LaneScorer(self.spectra), nlive, ndata, sample.kernel_params)
            xs0 = sample.priortransform_batch(rng.uniform(size=(nlive, 3)))
            self.dev.init(xs0)
            self.host.init(xs0)
            self.nlive = nlive
        else:
            # the scale-marginalised likelihood of the MUSE-style problem: five parameters, no numpy statement here
            from massivedatans_amd import gen, musefuse
            from massivedatans_amd.like import MuseSpectra
            data = gen.muse_like(ndata, nx)
            self.spectra = MuseSpectra(data["x"], data["y"], data["v"])
            self.dev = jointstate.MuseJointState(self.spectra, nlive)
            self.dev.init(musefuse.priortransform_batch(rng.uniform(size=(nlive, 5))))
            self.nlive = nlive

    def set_thresholds(self, thr):
        """Thresholds planted: live row 0 carries them, the other rows lie above."""
        live = np.tile(np.asarray(thr, dtype=float) + np.abs(thr) * 0.5 + 1.0, (self.nlive, 1))
        live[0] = thr
        live = np.ascontiguousarray(live)
        call(self.lib.mdns_joint_set_live(self.dev._h, _lib.ptr(live)), "mdns_joint_set_live")
        self.host.live = live.copy()

    def prepare(self):
        a, b = self.dev.prepare(), self.host.prepare()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    def statement(self, prior, limit, metric, pow10):
        mean, scale = metric if metric is not None else (None, None)
        return constrainer.chain_statement(self.u, self.mn, self.mx, self.radius, self.ms.count, mean, scale, prior, limit, pow10=pow10)

    def chain(self, prior, limit, metric, rows, begin_draw=True):
        """region_begin (K6 in flight), draw_begin, chain_begin, chain_end, region_radius on the device."""
        lib, dev = self.lib, self.dev
        M = self.ndata if rows is None else len(rows)
        region = lib.mdns_backend_region_begin(dev._h, _lib.ptr(self.members), self.K, self.ndim, _lib.ptr(self.masks), NBOOT)
        assert region, _lib.last_error()
        try:
            if begin_draw:
                call(lib.mdns_backend_draw_begin(dev._h, _lib.ptr(rows) if rows is not None else None, M), "draw_begin")
            mean, scale = metric if metric is not None else (None, None)
            rq = make_request(self.u, self.mn, self.mx, prior, limit, mean, scale)
            call(entry("chain_begin")(dev._h, region, C.addressof(rq)), "chain_begin")
            counts = np.full(self.n, -7, dtype=np.int32)
            nkept, B, accepted = C.c_int(-9), C.c_int(-9), C.c_int(-9)
            bits = np.zeros((M + 63) // 64 + 1, dtype=np.uint64)
            params = np.full((1024, 3), np.nan)
            ip = C.POINTER(C.c_int)
            call(entry("chain_end")(dev._h, region, counts.ctypes.data_as(ip), C.byref(nkept), C.byref(B), C.byref(accepted),
                                    bits.ctypes.data_as(C.POINTER(C.c_ulonglong)), params.ctypes.data_as(C.POINTER(C.c_double))), "chain_end")
            radius = C.c_double(0)
            call(lib.mdns_backend_region_radius(dev._h, region, C.byref(radius)), "region_radius")
        finally:
            lib.mdns_backend_region_destroy(dev._h, region)
        beats = np.unpackbits(bits[:(M + 63) // 64].view(np.uint8), bitorder='little')[:M].astype(bool)
        return dict(counts=counts, nkept=nkept.value, B=B.value, accepted=accepted.value, beats=beats, params=params, radius=radius.value)

    def close(self):
        if hasattr(self, "dev"):
            self.dev.close()
        self.ms.close()


def check_case(s, oracle, pow10_dd, prior, limit, metric=None, rows=None, plant=None, expect_full=True, follow_up=True):
    """One chained batch against the statement; returns what the device answered (and the statement's kept
    count) so that a case can assert it reached the code it names.  The parameters are compared bit for bit
    for every candidate; the check against the CORRECTLY ROUNDED values (within one ulp) looks at the first
    40 candidates only (the 60-digit power is slow) and not at all at a prior that takes 10** twice on one
    dimension, where an ulp of the inner power is many of the outer."""
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
    cap = min(limit, 1024)
    props, counts, kept, want = s.statement(prior, cap, metric, pow10_dd)
    # the statement's counts are K3's on its own proposals; the CPU oracle agrees
    assert np.array_equal(counts, oracle.count_within_distance_of(s.members, s.radius, props).astype(np.int32))
    nkept = int(kept.sum())
    if plant is not None and expect_full and cap > 0 and len(want):
        sel = np.arange(s.ndata) if rows is None else rows
        mask = np.zeros(s.ndata, dtype=bool)
        mask[sel] = True
        Lall = LaneScorer(s.spectra).loglike_batch(want, mask)           # the lane kernel's values [B, M]
        thr = np.full(s.ndata, 0.0)
        best = Lall.max(axis=0)
        thr[sel] = best + np.abs(best) * 1e-3                              # nobody is accepted ...
        if plant != "nobody":
            # ... but candidate b, on a data set where it is the best of the chunk
            kind, b = plant
            b = min(b, len(want) - 1)
            d = int(np.argmax(Lall[b] - np.delete(Lall, b, axis=0).max(axis=0))) if len(want) > 1 else 0
            thr[sel[d]] = Lall[b, d] if kind == "on" else np.nextafter(Lall[b, d], -np.inf)
        s.set_thresholds(thr)
    s.prepare()
    before = s.dev.thresholds()
    got = s.chain(prior, limit, metric, rows)
    assert got["radius"] == s.radius                                        # K6 in flight gave the synchronous call's radius
    assert np.array_equal(got["counts"], counts), np.flatnonzero(got["counts"] != counts)[:10]
    if not (expect_full and cap > 0):
        assert got["nkept"] == -1 and got["B"] == 0 and got["accepted"] == -1
        after = s.dev.thresholds()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        return got, nkept
    assert got["nkept"] == nkept and got["B"] == min(nkept, cap), (got["nkept"], got["B"], nkept, cap)
    B = got["B"]
    dev_params = got["params"][:B]
    assert np.array_equal(dev_params.view(np.int64), want.view(np.int64)), \
        ("parameters differ from the statement's", np.argwhere(dev_params != want)[:5])
    if B == 0:
        assert got["accepted"] == -1
        after = s.dev.thresholds()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        return got, nkept
    v = props[kept][:B] if metric is None else (props * metric[1] + metric[0])[kept][:B]
    import decimal

    def exact(x):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return np.array([float(decimal.Decimal(10) ** decimal.Decimal(float(t))) for t in x])
    few = slice(0, min(B, 40))
    twice = any(prior.pow10[k] and prior.kernel_pow10[k] for k in range(min(3, prior.ndim)))
    if not twice:                                                           # (10**(10**v): an ulp of the inner power is many of the outer)
        assert ulps_apart(dev_params[few], constrainer.chain_params(v[few], prior, exact)).max() <= 1
    idx, _, beats, _ = s.host.draw_params(dev_params, rows)
    assert got["accepted"] == idx, (got["accepted"], idx)
    if idx >= 0:
        assert np.array_equal(got["beats"], beats)
        s.dev.took(rows, got["beats"])
    ha, na = s.dev.thresholds()
    hb, nb = s.host.thresholds()
    assert np.array_equal(na, nb) and np.array_equal(ha, hb)
    if follow_up:
        # an ordinary chunk on the same handle afterwards: the chain left selection, shelves and trail usable
        ordinary_draw(s, rows)
        s.prepare()
        ha, na = s.dev.thresholds()
        hb, nb = s.host.thresholds()
        assert np.array_equal(na, nb) and np.array_equal(ha, hb)
    return got, nkept


def ordinary_draw(s, rows=None):
    """A chunk through mdns_backend_draw_begin / _chunk on both states, then the thresholds of both."""
    cube = s.rng.uniform(size=(37, 3))
    cube[:, 0] *= 0.2
    p2 = sample.kernel_params(sample.priortransform_batch(cube))
    ia, _, ba, _ = s.dev.draw_params(p2, rows)
    ib, _, bb, _ = s.host.draw_params(p2, rows)
    assert ia == ib
    if ia >= 0:
        assert np.array_equal(ba, bb)
    ha, na = s.dev.thresholds()
    hb, nb = s.host.thresholds()
    assert np.array_equal(na, nb) and np.array_equal(ha, hb)


def same_thresholds(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def shrinking_metric(s, share=0.5):
    """A scaling metric (sdml.py: x = y * scale + mean) whose inverse image leaves about ``share`` of the box
    inside the unit cube in the first dimension."""
    scale = np.ones(s.ndim)
    mean = np.zeros(s.ndim)
    scale[0] = 3.0
    mean[0] = -3.0 * 0.5 + 0.5 + (0.5 - share) * 1.0
    return mean, scale


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [1, 2, 3, 4, 5])
def test_every_dimension_of_the_box_kernel(child, oracle, pow10_dd, ndim):
    """k_box_count<D> for D = 1..5; with fewer than three dimensions the missing kernel parameters are 0."""
    if child():
        return
    s = Setup(ndim=ndim, n=1000, K=150 + ndim)
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(ndim), 64, follow_up=ndim >= 3)
    assert nkept > 64 and got["B"] == 64
    s.close()


def test_six_dimensions_are_refused(child):
    if child():
        return
    s = Setup(ndim=6, n=100, K=60)
    s.prepare()
    lib, dev = s.lib, s.dev
    before = dev.thresholds()
    region = lib.mdns_backend_region_begin(dev._h, _lib.ptr(s.members), s.K, 6, _lib.ptr(s.masks), NBOOT)
    assert region, _lib.last_error()
    call(lib.mdns_backend_draw_begin(dev._h, None, s.ndata), "draw_begin")
    rq = make_request(s.u, s.mn, s.mx, prior_of(6), 8)
    assert entry("chain_begin")(dev._h, region, C.addressof(rq)) != 0
    assert "6 dimensions" in _lib.last_error()
    assert same_thresholds(before, dev.thresholds())
    radius = C.c_double(0)
    call(lib.mdns_backend_region_radius(dev._h, region, C.byref(radius)), "region_radius")
    assert radius.value == s.radius
    lib.mdns_backend_region_destroy(dev._h, region)
    ordinary_draw(s)
    s.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1000, 1024])
def test_number_of_proposals(child, oracle, pow10_dd, n):
    """Workgroups of four proposals with a ragged last one; the 256-wide ranking loop and its running base."""
    if child():
        return
    s = Setup(n=n, K=120)
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3), 1024)
    assert got["B"] == nkept
    if n >= 255:
        assert nkept > 4
    s.close()


def test_more_than_1024_proposals_are_refused(child):
    if child():
        return
    s = Setup(n=1025, K=60)
    s.prepare()
    lib, dev = s.lib, s.dev
    before = dev.thresholds()
    region = lib.mdns_backend_region_begin(dev._h, _lib.ptr(s.members), s.K, 3, _lib.ptr(s.masks), NBOOT)
    assert region, _lib.last_error()
    call(lib.mdns_backend_draw_begin(dev._h, None, s.ndata), "draw_begin")
    rq = make_request(s.u, s.mn, s.mx, prior_of(3), 8)
    assert entry("chain_begin")(dev._h, region, C.addressof(rq)) != 0
    assert "1025 proposals" in _lib.last_error()
    assert same_thresholds(before, dev.thresholds())
    radius = C.c_double(0)
    call(lib.mdns_backend_region_radius(dev._h, region, C.byref(radius)), "region_radius")
    lib.mdns_backend_region_destroy(dev._h, region)
    ordinary_draw(s)
    s.close()


@pytest.mark.parametrize("K", [2, 63, 511, 512, 513, 1500])
def test_number_of_members(child, oracle, pow10_dd, K):
    """The LDS tile of 512 members and its 64 slices."""
    if child():
        return
    s = Setup(n=600, K=K)
    check_case(s, oracle, pow10_dd, prior_of(3), 32)
    s.close()


@pytest.mark.parametrize("limit,want", [(1, 1), (1, 4), (3, 1), (3, 3), (3, 6), (4, 2), (4, 4), (4, 7), (5, 3), (5, 5), (5, 8),
                                        (64, 62), (64, 64), (64, 67), (1024, None)])
def test_chunk_limit_against_the_kept_proposals(child, oracle, pow10_dd, limit, want):
    """``rank < limit`` and the tiles of four when the limit is not a multiple of four, with ``want`` kept
    proposals: fewer than, exactly as many as, and more than the limit (1024 proposals cannot keep more than
    a limit of 1024: there all of them are offered and all kept ones are candidates)."""
    if child():
        return
    s = Setup(n=1024, K=100, ndata=70)
    _, _, kept, _ = s.statement(prior_of(3), 0, None, None)
    order = np.flatnonzero(kept)
    assert len(order) > 70
    if want is None:
        want = len(order)
    else:
        # the batch ends just before the kept proposal number want + 1: the ones that are not kept in between stay
        s.n = int(order[want])
        s.u = np.ascontiguousarray(s.u[:s.n])
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3), limit)
    assert nkept == want and got["B"] == min(want, limit)
    s.close()


def test_no_proposal_is_kept(child, oracle, pow10_dd):
    """Every proposal maps outside the unit cube: nkept = 0, B = 0, nobody accepted, nothing changed."""
    if child():
        return
    s = Setup(n=500, K=100)
    metric = (np.array([0.0, 5.0, 0.0]), np.ones(3))
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3), 64, metric=metric)
    assert nkept == 0 and got["nkept"] == 0 and got["B"] == 0 and (got["counts"] > 0).sum() > 50
    # and the handle still draws
    p2 = sample.kernel_params(sample.priortransform_batch(s.rng.uniform(size=(20, 3)) * [0.1, 1, 1]))
    ia, _, ba, _ = s.dev.draw_params(p2, None)
    ib, _, bb, _ = s.host.draw_params(p2, None)
    assert ia == ib
    s.close()


def test_scaling_metric_and_the_strict_unit_cube(child, oracle, pow10_dd):
    """A scaling metric that leaves about half of the box outside the unit cube, shifted so that one kept-looking
    proposal lands EXACTLY on 0.0 in one dimension and another exactly on 1.0 in a second: both are outside."""
    if child():
        return
    s = Setup(n=1000, K=200, spread=0.3)
    props, counts, _, _ = s.statement(prior_of(3), 0, None, None)
    inside = np.flatnonzero((counts > 0) & ((props > 0.05) & (props < 0.95)).all(axis=1))
    i0 = int(inside[len(inside) // 2])
    i1 = int(inside[np.argmax((props[inside, 1] >= 0.5) & (inside != i0))])
    assert props[i1, 1] >= 0.5 and i1 != i0
    mean = np.array([-props[i0, 0], 1.0 - props[i1, 1], 0.0])
    scale = np.ones(3)
    v = props * scale + mean
    assert v[i0, 0] == 0.0 and v[i1, 1] == 1.0
    _, _, kept, _ = s.statement(prior_of(3), 0, (mean, scale), None)
    assert not kept[i0] and not kept[i1]
    share = 1.0 - kept.sum() / float((counts > 0).sum())
    assert 0.3 < share < 0.99, share
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3), 1024, metric=(mean, scale))
    assert got["B"] == nkept > 0
    # a true scaling as well
    s2 = Setup(n=1000, K=200, seed=1)
    got, nkept = check_case(s2, oracle, pow10_dd, prior_of(3), 100, metric=shrinking_metric(s2))
    assert 0 < nkept < (got["counts"] > 0).sum()
    s.close()
    s2.close()


@pytest.mark.parametrize("M", [1, 63, 64, 65, 128, 129, 4096])
@pytest.mark.parametrize("selection", ["all", "rows"])
def test_number_of_spectra(child, oracle, pow10_dd, M, selection):
    """Tiles of 64 spectra with a ragged last one; up to 128 selected spectra k_chunk_commit commits, above the
    trail commit; ``rows``: a ragged ascending selection out of more."""
    if child():
        return
    ndata = M if selection == "all" else M + max(3, M // 3)
    s = Setup(n=400, K=100, ndata=ndata, nlive=8)
    rows = None if selection == "all" else np.sort(s.rng.choice(ndata, size=M, replace=False))
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3), 24, rows=rows, plant=("below", 17))
    assert got["B"] == 24 and got["accepted"] >= 0
    s.close()


def test_more_than_4096_spectra_with_a_short_chunk(child, oracle, pow10_dd):
    if child():
        return
    s = Setup(n=300, K=100, ndata=4500, nlive=6)
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3), 8, plant=("below", 6))
    assert got["B"] == 8 and got["accepted"] >= 0
    # more than eight candidates over so many spectra do not ride along: counts only
    got, _ = check_case(s, oracle, pow10_dd, prior_of(3), 9, expect_full=False)
    s.close()


@pytest.mark.parametrize("nx", [1, 7, 64, 65, 128, 129, 200, 208, 209, 256])
def test_number_of_channels(child, oracle, pow10_dd, nx):
    """k_chain_accept<8 / 16 / 26 / 32> and their ragged tails."""
    if child():
        return
    s = Setup(n=500, K=100, nx=nx, ndata=130)
    got, _ = check_case(s, oracle, pow10_dd, prior_of(3), 16, plant=("below", 9))
    assert got["B"] == 16 and got["accepted"] >= 0
    s.close()


def test_too_many_channels_go_the_counts_only_way(child, oracle, pow10_dd):
    if child():
        return
    s = Setup(n=500, K=100, nx=257, ndata=40)
    check_case(s, oracle, pow10_dd, prior_of(3), 16, expect_full=False)
    s.close()


def test_limit_zero_is_counts_only(child, oracle, pow10_dd):
    if child():
        return
    s = Setup(n=1000, K=300)
    check_case(s, oracle, pow10_dd, prior_of(3), 0, expect_full=False)
    check_case(s, oracle, pow10_dd, prior_of(3), 0, expect_full=False, metric=shrinking_metric(s))
    s.close()


@pytest.mark.parametrize("kind", ["sample", "b0", "plain", "twice"])
def test_priors(child, oracle, pow10_dd, kind):
    if child():
        return
    s = Setup(n=1000, K=200, seed=3)
    got, nkept = check_case(s, oracle, pow10_dd, prior_of(3, kind), 200)
    assert got["B"] == min(nkept, 200) > 20
    s.close()


@pytest.mark.parametrize("plant", [("on", 1), ("below", 1), ("below", 6), ("below", 10), "nobody", ("on", 10)],
                         ids=["on-first", "below-first", "below-middle", "below-last", "nobody", "on-last"])
def test_thresholds_on_and_one_ulp_below_a_candidate(child, oracle, pow10_dd, plant):
    """A threshold exactly on a candidate's likelihood does not accept it (L > thr), one ulp below does;
    the candidate in the first, a middle and the last tile of four of a chunk of twelve."""
    if child():
        return
    s = Setup(n=800, K=150, ndata=300, seed=5, spread=0.45)
    got, _ = check_case(s, oracle, pow10_dd, prior_of(3, "lines"), 12, plant=plant)
    assert got["B"] == 12
    if plant == "nobody" or plant[0] == "on":
        assert got["accepted"] == -1
    else:
        assert got["accepted"] == plant[1] and got["beats"].sum() == 1
    s.close()


def test_two_chains_in_a_row_and_then_an_iteration(child, oracle, pow10_dd):
    """Mailbox sequence numbers and the reuse of the mapped block; thresholds so low that the accepted
    candidates fill every shelf, then advance / prepare on both states."""
    if child():
        return
    s = Setup(n=700, K=150, ndata=200, seed=7)
    s.set_thresholds(np.full(s.ndata, -1e12))
    got, _ = check_case(s, oracle, pow10_dd, prior_of(3), 40, follow_up=False)
    assert got["accepted"] == 0 and got["beats"].all()
    s.u = np.ascontiguousarray(s.rng.uniform(size=(s.n, 3)))
    got, _ = check_case(s, oracle, pow10_dd, prior_of(3), 33, follow_up=False, rows=np.arange(5, 150, 3))
    check_case(s, oracle, pow10_dd, prior_of(3), 0, expect_full=False)
    got, _ = check_case(s, oracle, pow10_dd, prior_of(3), 5)
    s.dev.advance()
    s.host.advance()
    s.prepare()
    assert np.array_equal(s.dev.live_matrix(), s.host.live_matrix())
    s.close()


def test_misuse_is_refused_with_a_message(child):
    """chain_begin without a draw begun, while a chain is in flight; chain_end with none in flight: refused, and
    the state is what it was -- after the refusals before the chain, and after the one chain that did run it
    is what the numpy statement has after the same chunk."""
    if child():
        return
    s = Setup(n=200, K=80)
    s.prepare()
    lib, dev = s.lib, s.dev
    before = dev.thresholds()
    region = lib.mdns_backend_region_begin(dev._h, _lib.ptr(s.members), s.K, 3, _lib.ptr(s.masks), NBOOT)
    assert region, _lib.last_error()
    rq = make_request(s.u, s.mn, s.mx, prior_of(3), 8)
    assert entry("chain_begin")(dev._h, region, C.addressof(rq)) != 0
    assert "no draw begun" in _lib.last_error()
    counts = np.zeros(s.n, dtype=np.int32)
    nkept, B, accepted = C.c_int(0), C.c_int(0), C.c_int(0)
    bits = np.zeros((s.ndata + 63) // 64 + 1, dtype=np.uint64)
    params = np.full((1024, 3), np.nan)
    ip = C.POINTER(C.c_int)

    def end():
        return entry("chain_end")(dev._h, region, counts.ctypes.data_as(ip), C.byref(nkept), C.byref(B), C.byref(accepted),
                                  bits.ctypes.data_as(C.POINTER(C.c_ulonglong)), params.ctypes.data_as(C.POINTER(C.c_double)))
    assert end() != 0
    assert "no chain in flight" in _lib.last_error()
    assert same_thresholds(before, dev.thresholds())
    call(lib.mdns_backend_draw_begin(dev._h, None, s.ndata), "draw_begin")
    call(entry("chain_begin")(dev._h, region, C.addressof(rq)), "chain_begin")
    assert entry("chain_begin")(dev._h, region, C.addressof(rq)) != 0
    assert "a chain is in flight" in _lib.last_error()
    call(end(), "chain_end")                                   # the chain in flight was not disturbed
    assert nkept.value >= B.value > 0
    took = accepted.value
    idx, _, beats, _ = s.host.draw_params(params[:B.value].copy(), None)
    assert took == idx
    if idx >= 0:
        got = np.unpackbits(bits[:(s.ndata + 63) // 64].view(np.uint8), bitorder='little')[:s.ndata].astype(bool)
        assert np.array_equal(got, beats)
        dev.took(None, got)
    assert same_thresholds(dev.thresholds(), s.host.thresholds())
    assert end() != 0
    assert "no chain in flight" in _lib.last_error()
    assert same_thresholds(dev.thresholds(), s.host.thresholds())
    radius = C.c_double(0)
    call(lib.mdns_backend_region_radius(dev._h, region, C.byref(radius)), "region_radius")
    lib.mdns_backend_region_destroy(dev._h, region)
    ordinary_draw(s)
    s.close()


def test_a_muse_joint_state_is_counts_only(child, oracle):
    """A joint state of the MUSE-style likelihood (``kind`` 1 in mdns_backend_chain_begin) chains proposals and
    membership counts only, whatever the request: here a request that a Gaussian-line state would serve in
    full (three kernel parameters, no noise, limit 16)."""
    if child():
        return
    s = Setup(ndim=5, n=700, K=150, nx=200, ndata=60, nlive=12, joint="muse")
    assert type(s.dev).__name__ == "MuseJointState"
    s.dev.prepare()
    before = s.dev.thresholds()
    for metric in (None, shrinking_metric(s)):
        props, counts, kept, _ = s.statement(prior_of(5), 0, metric, None)
        assert np.array_equal(counts, oracle.count_within_distance_of(s.members, s.radius, props).astype(np.int32))
        assert 0 < kept.sum() < s.n
        got = s.chain(prior_of(5), 16, metric, None)
        assert got["radius"] == s.radius
        assert np.array_equal(got["counts"], counts)
        assert got["nkept"] == -1 and got["B"] == 0 and got["accepted"] == -1
        assert same_thresholds(before, s.dev.thresholds())
    # and the handle still draws
    from massivedatans_amd import musefuse
    idx, _, _, nscored = s.dev.draw_params(musefuse.priortransform_batch(s.rng.uniform(size=(9, 5))), None)
    assert nscored == 9 and -1 <= idx < 9
    s.close()


def test_whole_run_with_and_without_the_chain(child, monkeypatch):
    """The same analysis (horns, 300 data sets, 50 live points, 500 iterations, native core) with the chained
    first batches and with MDNS_CHAIN=0: the chained path scores its candidates with ``pow10_dd`` parameters,
    the unchained one with the C library's, so likelihoods may differ in their last bits; iterations, draws and
    the accepted points (the host's arithmetic on both paths) must be identical and the evidences agree to
    the 1e-9 the README states for device against CPU path."""
    if child():
        return
    from massivedatans_amd import gen
    data = gen.horns(300)
    runs = []
    for chain in ("1", "0"):
        monkeypatch.setenv("MDNS_CHAIN", chain)
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run(data["x"], data["y"], nlive_points=50, max_samples=500)
        assert type(sampler).__name__ == "NativeCoreSampler" and sampler.native is not None
        st = sampler.native.stats()
        print("MDNS_CHAIN=%s: %d chains, %d counts-only, %d draws, %d accepted candidates with device parameters not the host's"
              % (chain, st["chains"], st["chain_counts"], st["draws"], st["param_mismatch"]))
        assert (st["chains"] > 0) == (chain == "1")
        if chain == "0":
            assert st["chain_counts"] == 0 and st["param_mismatch"] == 0
        runs.append((results, sampler.ndraws, np.array(sampler.pointpile, dtype=np.float64), st["draws"]))
    (ra, na, pa, da), (rb, nb, pb, db) = runs
    assert ra["nsamples"] == rb["nsamples"] and na == nb and da == db
    assert pa.shape == pb.shape and np.array_equal(pa, pb)
    assert len(ra["weights"]) == len(rb["weights"])
    assert np.max(np.abs(np.asarray(ra["logZ"]) - np.asarray(rb["logZ"]))) < 1e-9
