"""The cases test_filter_shapes.py runs under every mode of the guarded accept filters, each mode in a child
pytest process over this file (the library reads MDNS_K1_FILTER* once per process; filter_support.child_environment).
Not collected with the suite: the file name keeps it out, and outside such a child every case fails at once.

Part A plants decisions over filter_support.SHAPES and compares them with a plain numpy statement in np.longdouble;
Part B runs test_joint.py's whole-state comparison with a filter deciding the chunks; Part C overflows the list of
the exact re-score behind the matrix-core forms."""
import os

import numpy as np
import pytest

from massivedatans_amd import _lib, gen, jointstate, sample
from massivedatans_amd.like import GaussLineSpectra
from chain_support import LaneScorer
import filter_support as fs

pytestmark = pytest.mark.gpu

MODE = os.environ.get(fs.MODE_VARIABLE)
NLIVE = 3
FILLER = 1e300          # live points nobody looks at: above every likelihood


@pytest.fixture(autouse=True)
def _in_a_child():
    assert MODE in fs.MODES, "these cases run in a child of test_filter_shapes.py (%s names the mode)" % fs.MODE_VARIABLE
    for k, v in fs.child_environment(MODE).items():
        if k.startswith("MDNS_K1_") or k == "MDNS_CHUNK_PATH":
            assert os.environ.get(k) == v, (k, os.environ.get(k), v)


def _kernel(hip):
    return (hip.mdns_profile_kernel(0) or b"").decode()


class _Planted(object):
    """One joint state over the spectra of a shape; ``run`` plants thresholds, draws the shape's chunk on its
    selection and returns the outcome with the thresholds and shelf sizes afterwards."""

    def __init__(self, hip, spectra, params, rows, nx, fetch_rows):
        self.hip, self.params, self.rows, self.nx = hip, params, rows, nx
        self.js = jointstate.GaussJointState(spectra, NLIVE, lambda p: p, fetch_rows=fetch_rows)

    def run(self, thr):
        live = np.full((NLIVE, len(thr)), FILLER)
        live[0] = thr
        _lib.check(self.hip.mdns_joint_set_live(self.js._h, _lib.ptr(np.ascontiguousarray(live))), "set_live")
        self.js.prepare()
        before, n0 = self.js.thresholds()
        assert np.array_equal(before, thr) and not n0.any()
        idx, Lrow, beats, n = self.js.draw_params(self.params, self.rows)
        name = _kernel(self.hip)
        assert name.startswith(fs.expected_kernel(MODE, self.nx)), ("the kernel of this mode did not score the chunk", name)
        assert n == len(self.params)
        after, n1 = self.js.thresholds()
        return idx, Lrow, beats, after, n1

    def close(self):
        self.js.close()


def _check_outcome(got, thr, rows, L, Lall):
    """The outcome of a draw against the decision ``L`` [B, ndata] gives under thresholds ``thr``: index, fill bits
    position by position, the kept row, thresholds and shelf sizes afterwards (untouched outside the selection).
    ``Lall``: the chain's values, which everything kept must equal bit for bit."""
    idx, Lrow, beats, after, n1 = got
    want_idx, want_beats = fs.decision(L, thr, rows)
    assert idx == want_idx, (idx, want_idx)
    sel = np.arange(len(thr)) if rows is None else rows
    want_thr, want_n = thr.copy(), np.zeros(len(thr), dtype=int)
    if idx >= 0:
        assert np.array_equal(beats, want_beats), np.flatnonzero(beats != want_beats)
        if Lrow is not None:
            assert np.array_equal(Lrow, Lall[idx, sel])
            assert np.all(np.abs(Lrow - L[idx, sel]) <= fs.RTOL_L * np.abs(L[idx, sel]))
        # one point waiting: the threshold is the second smallest of {thr, the point, the fillers}: the point
        want_thr[sel[want_beats]] = Lall[idx, sel[want_beats]]
        want_n[sel[want_beats]] = 1
    else:
        assert Lrow is None and beats is None
    assert np.array_equal(n1, want_n)
    assert np.array_equal(after, want_thr)
    changed = sel[want_beats] if idx >= 0 else sel[:0]
    assert np.all(np.abs(after[changed] - L[idx, changed].astype(np.float64)) <= fs.RTOL_L * np.abs(after[changed]))


@pytest.mark.parametrize("shape", fs.SHAPES, ids=fs.shape_id)
def test_planted_decisions(hip, shape):
    """Base, tie, one ulp below the tie, ordinary and offset-data cases of one shape (the issue's Part A), with
    the likelihood row fetched (commit by k_gauss_cols_commit) and not (commit from the trail)."""
    ndata, _, nx, B = shape
    for offset in (0.0, 3.0):
        x, y, params, rows, L_ref = fs.reference(shape, offset)
        M = ndata if rows is None else len(rows)
        sel = np.arange(ndata) if rows is None else rows
        spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
        # 1. the chain's values against the plain statement
        Lall = LaneScorer(spectra).loglike_batch(params)
        assert Lall.shape == (B, ndata)
        # (RTOL_L pair by pair, as test_hip_parity.py asks; only where the float64 templates of the reference decide
        # less than a tenth of that themselves -- a template that meets a spectrum of one or a few channels almost
        # exactly -- their resolution is added: filter_support.reference_resolution)
        err = np.abs(Lall - L_ref) / np.abs(L_ref)
        res = fs.reference_resolution(x, y, params)
        blurred = res > 0.1 * fs.RTOL_L * np.abs(L_ref)
        print("%s offset %g: chain against L_ref %.3g; %d of %d pairs blurred by the reference's templates, the others %.3g"
              % (fs.shape_id(shape), offset, float(err.max()), int(blurred.sum()), blurred.size, float(err[~blurred].max())))
        assert nx < 7 or not blurred.any()
        assert (np.abs(Lall - L_ref) <= fs.RTOL_L * np.abs(L_ref) + np.where(blurred, res, 0.0)).all(), float(err.max())
        base = fs.unbeatable(L_ref)
        ordinary = fs.ordinary_thresholds(L_ref, rows)
        for fetch_rows in (False, True):
            st = _Planted(hip, spectra, params, rows, nx, fetch_rows)
            # ordinary thresholds: some candidate is accepted, as the reference decides (offset 3.0: ysq is large
            # against msq - 2 S, the cancellation the 4 E band is there for)
            _check_outcome(st.run(ordinary), ordinary, rows, L_ref, Lall)
            if offset == 0.0:
                # thresholds nobody beats
                _check_outcome(st.run(base), base, rows, L_ref, Lall)
                # thresholds ON the chain value of the best candidate of six data sets: nobody (strict comparison)
                places = sorted(set(p for p in (0, M - 1, 15, 16, 63, 64) if p < M))
                planted = [(int(sel[p]), int(np.argmax(Lall[:, sel[p]]))) for p in places]
                thr = base.copy()
                for d, b in planted:
                    thr[d] = Lall[b, d]
                got = st.run(thr)
                assert got[0] == -1, got[0]
                _check_outcome(got, thr, rows, Lall, Lall)
                # one ulp below: the first planted candidate, with exactly the planted fill bits
                thr = base.copy()
                for d, b in planted:
                    thr[d] = np.nextafter(Lall[b, d], -np.inf)
                got = st.run(thr)
                first = min(b for _, b in planted)
                want = np.zeros(ndata, dtype=bool)
                for d, b in planted:
                    want[d] = Lall[first, d] > thr[d]
                assert got[0] == first and np.array_equal(got[2], want[sel]) and got[2].sum() >= 1
                _check_outcome(got, thr, rows, Lall, Lall)
            st.close()


def _horns_spectra(ndata, nx):
    data = gen.horns(ndata)
    x = np.linspace(400, 800, nx) if nx > 200 else data["x"][:nx]
    y = np.ascontiguousarray(np.vstack([data["y"]] * (-(-nx // 200)))[:nx])
    return GaussLineSpectra(x, y, noise_level=0.01)


@pytest.mark.parametrize("fetch_rows", [True, False, "backend"])
@pytest.mark.parametrize("ndata,nlive,nx", [(700, 30, 201), (90, 150, 48), (300, 20, 300)])
def test_joint_state_under_a_filter(hip, ndata, nlive, nx, fetch_rows):
    """test_joint.py's test_joint_state_equals_its_numpy_statement with the filter of this mode deciding the
    chunks: exact equality with HostJointState over the lane kernel, through commits from the trail and with a
    fetched row behind gathered filter passes, shelf growth and set_running; and at least half of the chunks of 8+
    candidates scored by the kernel of this mode."""
    rng = np.random.RandomState(ndata * 7 + nlive)
    spectra = _horns_spectra(ndata, nx)
    dev = fs.CountingState(jointstate.GaussJointState(spectra, nlive, sample.kernel_params, shelf_cap=4, fetch_rows=fetch_rows is True,
                                                      via_backend=fetch_rows == "backend"), hip)
    host = jointstate.HostJointState(LaneScorer(spectra), nlive, ndata, sample.kernel_params)
    xs0 = sample.priortransform_batch(rng.uniform(size=(nlive, 3)))
    dev.init(xs0)
    host.init(xs0)
    assert np.array_equal(dev.live_matrix(), host.live_matrix())
    ndraws = fs._drive(dev, host, ndata, rng, iterations=12, exact=True)
    assert ndraws > 0
    name = fs.expected_kernel(MODE, nx)
    large = sum(1 for B, _ in dev.chunks if B >= 8)
    scored = sum(1 for _, k in dev.chunks if k.startswith(name))
    print("%d chunks, %d of 8+ candidates, %d scored by %s" % (len(dev.chunks), large, scored, name))
    assert large > 0 and 2 * scored >= large, (name, scored, large, sorted(set(k for _, k in dev.chunks)))
    dev.close()


def test_more_ambiguous_candidates_than_the_list_holds(hip):
    """80 candidates with the same parameters, thresholds exactly on their chain likelihood for one data set and
    unbeatable elsewhere: all 80 are ambiguous and none has a clear vote, the exact re-score lists 64 at the most --
    the draw must end in an error that names the guarded filter, not in a decision.  (The vector-FMA form resolves
    its ambiguous pairs in place and has no list: it must decide -- nobody is accepted.)"""
    ndata, nx, B = 300, 200, 80
    x, y, params, _ = fs.make_inputs((ndata, None, nx, B))
    params = np.ascontiguousarray(np.tile(params[:1], (B, 1)))
    spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
    Lall = LaneScorer(spectra).loglike_batch(params)
    assert (Lall == Lall[0]).all()
    thr = Lall[0] + np.abs(Lall[0]) * 1e-3
    thr[137] = Lall[0, 137]
    js = jointstate.GaussJointState(spectra, NLIVE, lambda p: p, fetch_rows=False)
    live = np.full((NLIVE, ndata), FILLER)
    live[0] = thr
    _lib.check(hip.mdns_joint_set_live(js._h, _lib.ptr(np.ascontiguousarray(live))), "set_live")
    js.prepare()
    if MODE == "1":
        idx, _, _, n = js.draw_params(params, None)
        assert idx == -1 and n == B and _kernel(hip).startswith(fs.expected_kernel(MODE, nx))
    else:
        with pytest.raises(_lib.MdnsError, match="guarded filter"):
            js.draw_params(params, None)
        assert _kernel(hip).startswith(fs.expected_kernel(MODE, nx))
        assert b"guarded filter" in hip.mdns_last_error()
    js.close()
