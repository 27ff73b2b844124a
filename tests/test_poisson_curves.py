"""The Poisson likelihood of count spectra on the GPU (csrc/mdns_curves.hip k_curve_log + k_curve_rows_p, include/mdns.h
Part 10): the kernels against the longdouble statement within the derived bound and -- with the device's own logarithms
read back through the kernel itself -- against the emulated chain bit for bit, the one value of a (curve, spectrum)
pair, the zero, invalid and masked rules to the bit, the joint state and a whole run against their numpy statements
over the same scores, what is refused, and that a handle without the mode scores as before."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, MuseSpectra, _Spectra
from curves_support import Chunks, StatementProblem, dev_batch, gauss_prior, line_model, refused, selections
from filter_support import _drive
from poisson_support import LOG_ULPS, TINY, DeviceScorer, NumpyPoisson, chain, count_data, count_model, within_bound

pytestmark = pytest.mark.gpu

NX = (1, 2, 31, 32, 33, 64, 200, 513)
NDATA = (1, 3, 70, 300)
BS = (1, 7, 8, 9, 32, 33, 70)
MS = (1, 64, 65, 128, 129)
# 16 + 2 cases: every nx twice, every ndata four times, every B at least twice, paired (no product); exposures given in the
# even cases, NULL in the odd ones
CASES = [(NX[i % 8], NDATA[(i + i // 8) % 4], BS[(3 * i + i // 8) % 7], i % 2 == 0) for i in range(16)]
CASES += [(513, 70, 33, True), (200, 300, 70, False)]         # and the largest of each together


def test_the_cases_cover_every_size():
    assert {c[0] for c in CASES} == set(NX) and {c[1] for c in CASES} == set(NDATA) and {c[2] for c in CASES} == set(BS)
    assert {c[3] for c in CASES} == {True, False} and len(set(CASES)) == 18
    # the sparse selections of MS need more spectra than they select: the cases with 300 spectra carry them
    assert sum(1 for c in CASES if c[1] == 300) >= 2


def _curves(B, nx, seed):
    """Count rates between 0.01 and 60 with a few exact zeros (of either sign)."""
    rng = np.random.RandomState(seed)
    curves = 10 ** rng.uniform(-2, np.log10(60.0), size=(B, nx))
    curves[rng.uniform(size=curves.shape) < 0.02] = 0.0
    curves[rng.uniform(size=curves.shape) < 0.01] = -0.0
    return curves


class _RawCounts(_Spectra):
    """A handle put into counts mode through the raw ABI: ``y``, ``e`` [nx, ndata] as they are, ``offsets`` or NULL."""

    def __init__(self, x, y, e=None, offsets=None):
        super(_RawCounts, self).__init__(x, y, None)
        rows = None if e is None else np.ascontiguousarray(np.asarray(e, dtype=float).T)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=float)
        _lib.check(self._lib.mdns_spectra_set_counts(self._h, _lib.ptr(rows) if rows is not None else None,
                                                     _lib.ptr(off) if off is not None else None), "mdns_spectra_set_counts")

    def poisson(self, curves, rows=None):
        return self._batch(self._lib.mdns_curve_poisson_batch, "mdns_curve_poisson_batch", np.atleast_2d(_lib.as_f64(curves)), rows)


def device_log(curves):
    """The ``lc`` k_curve_log makes of ``curves`` [B, nx] (finite, >= 0), read back exactly through the kernels
    themselves: spectrum k of the probe holds one count in channel k at an exposure of 2**-1000 and K = 0, so its chain
    is fma(-2**-1000, c_k, fma(1, lc_k, +0)) = lc_k -- the product is far below half an ulp of any lc != 0 (|lc| >=
    2**-53 for a double c != 1), and for lc = 0 what comes out is -2**-1000 c, recognised by its size."""
    B, nx = curves.shape
    probe = _RawCounts(np.arange(nx, dtype=float), np.eye(nx), 2.0 ** -1000 * np.eye(nx))
    lc = probe.poisson(curves)
    probe.close()
    assert lc.shape == (B, nx) and not np.isnan(lc).any()
    lc[np.abs(lc) < 1e-250] = 0.0
    return lc


@pytest.mark.parametrize("nx,ndata,B,exposure", CASES)
def test_kernel_against_the_statement(nx, ndata, B, exposure, hip):
    """Every L within ``bound`` of the longdouble statement (poisson_support derives it), over the whole set and over
    sparse selections of 1, 64, 65, 128 and 129 spectra, both entry points the same bits; the device's logarithms within
    LOG_ULPS ulps of the longdouble ones; and some pairs bit-equal to the chain emulated with those logarithms."""
    rng = np.random.RandomState(nx * 1000 + B)
    d = count_data(ndata, nx, seed=2, exposure=exposure)
    st = NumpyPoisson(d["y"], d["e"])
    spectra = CountSpectra(d["x"], d["y"], d["e"])
    assert hip.mdns_spectra_counts(spectra.handle) == 1 and np.array_equal(spectra.n_masked, st.n_masked) and spectra.continuum == 0
    curves = _curves(B, nx, nx + B)
    want = (st.loglike_batch_long(curves),) + st.sums_long(curves)        # once, for every selection
    worst = 0.0
    for name, rows in selections(ndata, rng, MS):
        got = spectra.loglike_batch_curves(curves, rows)
        assert got.shape == (B, ndata if rows is None else len(rows))
        ok, frac = within_bound(got, st, nx, curves, rows, want)
        worst = max(worst, frac)
        assert ok, (name, frac)
        assert np.array_equal(dev_batch(hip, spectra, curves, 3, rows, "mdns_curve_poisson_batch_dev"), got), name
        assert np.array_equal(spectra.loglike_batch(curves, rows), got), name
    lc = device_log(curves)
    exact = np.log(np.fmax(np.abs(curves), TINY).astype(np.longdouble))
    ulps = float((np.abs(lc.astype(np.longdouble) - exact) / np.spacing(np.abs(exact.astype(np.float64)))).max())
    print("nx=%d ndata=%d B=%d exposure=%s: worst error %.3g of the bound; device log within %.3g ulp" % (nx, ndata, B, exposure, worst, ulps))
    assert ulps <= LOG_ULPS
    whole = spectra.loglike_batch_curves(curves)
    for b, k in {(0, 0), (B - 1, ndata - 1), (B // 2, ndata // 2), (B - 1, ndata // 3), (0, 2 * ndata // 3)}:
        assert whole[b, k] == chain(curves[b], st.y[:, k], st.e[:, k], st.K[k], lc=lc[b]), (b, k)
    spectra.close()


def test_a_pair_has_one_value(hip):
    """The same bits for (curve b, spectrum k) in a batch of 70 x 300, alone, in a permuted batch over a sparse
    selection, through the device entry with another row stride, and in the live matrix of a joint state."""
    rng = np.random.RandomState(11)
    nx, ndata, B = 200, 300, 70
    d = count_data(ndata, nx, seed=4)
    curves = _curves(B, nx, 4)
    spectra = CountSpectra(d["x"], d["y"], d["e"])
    whole = spectra.loglike_batch_curves(curves)
    assert np.isfinite(whole).all()
    for b, k in [(0, 0), (69, 299), (31, 63), (32, 64), (33, 127), (8, 128), (7, 256), (64, 129)]:
        alone = spectra.loglike_batch_curves(curves[b:b + 1], np.array([k]))
        assert alone.shape == (1, 1) and np.array_equal(alone[0, 0], whole[b, k]), (b, k)
    perm = rng.permutation(B)
    sel = np.sort(rng.choice(ndata, size=137, replace=False))
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm], sel), whole[perm][:, sel])
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm[:5]], sel[3:4]), whole[perm[:5]][:, sel[3:4]])
    for pad in (0, 1, 56):
        assert np.array_equal(dev_batch(hip, spectra, curves[perm], pad, sel, "mdns_curve_poisson_batch_dev"), whole[perm][:, sel]), pad
    nlive = 40
    js = jointstate.CurveJointState(spectra, nlive, lambda xs: curves[xs[:, 0].astype(int)])
    js.init(np.arange(20, 20 + nlive, dtype=float)[:, None])
    assert np.array_equal(js.live_matrix(), whole[20:20 + nlive])
    js.close()
    spectra.close()


@pytest.mark.parametrize("name,bad", [("first", [0]), ("last", [47]), ("stage", list(range(16, 32))), ("scattered", [1, 15, 16, 32, 46]),
                                      ("all but one", [j for j in range(48) if j != 20])])
def test_a_masked_pixel_is_a_deleted_channel(name, bad):
    """e = 0 (or NaN, or a NaN count) in some channels of every spectrum: the bits of the same data with those channels
    deleted, whatever the curve says there."""
    nx, ndata, B = 48, 70, 9
    d = count_data(ndata, nx, seed=6, edges=False)
    curves = _curves(B, nx, 6)
    y, e = d["y"].copy(), d["e"].copy()
    e[bad[0::3]] = 0.0
    e[bad[1::3]] = np.nan
    y[bad[2::3]] = np.nan
    keep = np.setdiff1d(np.arange(nx), bad)
    with_mask = CountSpectra(d["x"], y, e)
    deleted = CountSpectra(d["x"][keep], np.ascontiguousarray(d["y"][keep]), np.ascontiguousarray(d["e"][keep]))
    assert (with_mask.n_masked - deleted.n_masked == len(bad)).all()
    wild = curves.copy()
    wild[:, bad] = 10 ** np.random.RandomState(7).uniform(-300, 300, size=(B, len(bad)))
    a = with_mask.loglike_batch_curves(curves)
    assert np.array_equal(a, deleted.loglike_batch_curves(np.ascontiguousarray(curves[:, keep]))) and np.isfinite(a).all()
    assert np.array_equal(a, with_mask.loglike_batch_curves(wild))
    with_mask.close()
    deleted.close()


def test_the_edges_to_the_bit(hip):
    """The fully masked spectrum scores +0.0; the all-zero one -sum e c by the chain; c = 0 (either sign) where n = 0
    nothing and where n > 0 n log(tiny) as the device rounds it; a negative and a NaN curve value NaN for every selected
    spectrum and for no other candidate of the batch."""
    nx, ndata, B = 33, 70, 9
    d = count_data(ndata, nx, seed=8)
    d["e"][5, 0] = 0.0                                                    # (a masked pixel in spectrum 0)
    st = NumpyPoisson(d["y"], d["e"])
    spectra = CountSpectra(d["x"], d["y"], d["e"])
    zero, gone = ndata // 3, 2 * ndata // 3
    assert spectra.n_masked[gone] == nx and st.K[gone] == 0 and st.K[zero] == 0 and not st.y[:, zero].any()
    curves = _curves(B, nx, 8)
    L = spectra.loglike_batch_curves(curves)
    assert (L[:, gone] == 0).all() and not np.signbit(L[:, gone]).any()
    lc = device_log(curves)
    for b in range(B):
        assert L[b, zero] == chain(curves[b], st.y[:, zero], st.e[:, zero], 0.0, lc=lc[b]) and L[b, zero] < 0
    # (the all-zero spectrum does not see the logarithms at all)
    assert np.array_equal(L[:, zero], [chain(curves[b], st.y[:, zero], st.e[:, zero], 0.0) for b in range(B)])
    # the zero model: a probe of four channels, counts (0, 3, 0, 2), exposures (1, 2, 0.5, 1.5), K = 0
    n, e = np.array([[0.0], [3.0], [0.0], [2.0]]), np.array([[1.0], [2.0], [0.5], [1.5]])
    probe = _RawCounts(np.arange(4.0), n, e)
    log_tiny = device_log(np.array([[0.0]]))[0, 0]
    assert abs(log_tiny - np.log(TINY)) <= LOG_ULPS * np.spacing(abs(np.log(TINY))) and log_tiny < -708
    c = np.array([[0.0, 0.25, -0.0, 1.0],          # c = +-0 where n = 0: nothing
                  [0.25, 0.0, 1.0, 1.0],           # c = +0 where n = 3
                  [0.25, -0.0, 1.0, 1.0],          # c = -0 where n = 3
                  [0.0, 0.0, 0.0, 0.0]])
    Lp = probe.poisson(c)[:, 0]
    lc4 = device_log(np.abs(c))
    assert np.array_equal(Lp, [chain(c[b], n[:, 0], e[:, 0], 0.0, lc=lc4[b]) for b in range(4)])
    assert Lp[0] == chain(c[0, [1, 3]], n[[1, 3], 0], e[[1, 3], 0], 0.0, lc=lc4[0, [1, 3]])
    assert Lp[1] == Lp[2] and np.isfinite(Lp).all() and Lp[3] < Lp[1] < -2100
    assert Lp[3] == 3 * log_tiny + 2 * log_tiny                           # (fma(2, lt, fl(3 lt)): 2 lt is exact)
    probe.close()
    # the invalid model
    sel = np.sort(np.random.RandomState(8).choice(ndata, size=40, replace=False))
    for bad in (-1e-300, -1.0, np.nan):
        for j in (0, nx - 1, 5):
            wrong = curves.copy()
            wrong[4, j] = bad
            for rows in (None, sel):
                Lw = spectra.loglike_batch_curves(wrong, rows)
                assert np.isnan(Lw[4]).all(), (bad, j)
                assert np.array_equal(np.delete(Lw, 4, axis=0), np.delete(L if rows is None else L[:, rows], 4, axis=0))
    spectra.close()


def test_raw_handle_with_and_without_exposures_and_offsets(hip):
    """mdns_spectra_set_counts through the raw ABI: NULL exposures are ones, NULL offsets zeros, and y is zeroed where
    e = 0 (the statement over the masked data gives the same bits as the class, which masks before it uploads)."""
    nx, ndata, B = 31, 70, 8
    d = count_data(ndata, nx, seed=9)
    y = np.where(np.isfinite(d["y"]), d["y"], 0.0)
    y[d["e"] == 0] = 3.0
    st = NumpyPoisson(y, d["e"])
    curves = _curves(B, nx, 9)
    cls = CountSpectra(d["x"], y, d["e"])
    raw = _RawCounts(d["x"], y, d["e"], st.K)             # (counts still in place under e = 0: the library zeroes them)
    assert np.array_equal(raw.poisson(curves), cls.loglike_batch_curves(curves))
    no_k = _RawCounts(d["x"], y, d["e"])
    assert np.array_equal(no_k.poisson(curves) + st.K[None, :], raw.poisson(curves))
    ones = _RawCounts(d["x"], y, None, None)
    given = _RawCounts(d["x"], y, np.ones_like(y), np.zeros(ndata))
    assert np.array_equal(ones.poisson(curves), given.poisson(curves))
    ok, frac = within_bound(ones.poisson(curves) + NumpyPoisson(y).K[None, :], NumpyPoisson(y), nx, curves)
    assert ok, frac
    for s in (cls, raw, no_k, ones, given):
        s.close()


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("ndata,nlive,nx", [(20, 8, 64), (130, 12, 33)])
def test_joint_state_equals_its_numpy_statement(ndata, nlive, nx, noisy):
    """CurveJointState over CountSpectra against HostJointState fed by mdns_curve_poisson_batch: accepted index, fill
    bits, thresholds and live matrix equal, over several prepare / draw / advance rounds, with and without jitter."""
    rng = np.random.RandomState(ndata * 7 + nlive + noisy)
    d = count_data(ndata, nx, seed=8, edges=False)
    spectra = CountSpectra(d["x"], d["y"], d["e"])
    model = count_model(d["x"])
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(DeviceScorer(spectra), nlive, ndata, model)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    noise0 = rng.normal(0, 1e-5, size=(nlive, ndata)) if noisy else None
    dev.init(xs0, jitter=noise0)
    host.init(xs0, jitter=noise0)
    assert dev.nparams == 3 and np.array_equal(dev.live_matrix(), host.live_matrix())
    want = NumpyPoisson(d["y"], d["e"]).loglike_batch_long(model(xs0)).astype(float) + (noise0 if noisy else 0)
    assert np.allclose(dev.live_matrix(), want, rtol=1e-11, atol=1e-9)
    assert _drive(Chunks(dev, lambda xs: xs, noisy), Chunks(host, model, noisy), ndata, rng, iterations=8, exact=True) > 0
    dev.close()
    spectra.close()


def test_whole_run_equals_the_statement():
    d = count_data(12, 64, seed=9, edges=False)
    x, y, e = d["x"], d["y"], d["e"]
    model = count_model(x)
    runs = []
    for cls in (problem.CurveProblem, StatementProblem):
        p = cls(x, y, model, gauss_prior, 3, poisson=True, exposure=e)
        assert isinstance(p.backend, CountSpectra)
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=20, max_samples=40, use_graph=False, seed=1)
        assert type(sampler.joint).__name__ == ("CurveJointState" if cls is problem.CurveProblem else "HostJointState")
        assert sampler.native is not None
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert runs[0][2] > 0 and runs[0][2] == runs[1][2] and np.isfinite(runs[0][0]).all()
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_the_mode_is_set_only_where_it_has_a_meaning(hip):
    nx, ndata = 64, 20
    d = count_data(ndata, nx, seed=10, edges=False)
    st = NumpyPoisson(d["y"], d["e"])
    rows = np.ascontiguousarray(st.e.T)
    curves = _curves(5, nx, 10)
    got = np.empty((5, ndata))
    assert hip.mdns_spectra_counts(None) == -1
    refused(hip.mdns_spectra_set_counts(None, None, None), "mdns_spectra_set_counts", "null")
    # a handle created with variances
    muse = MuseSpectra(d["x"], st.y, np.ones_like(st.y))
    refused(hip.mdns_spectra_set_counts(muse.handle, _lib.ptr(rows), None), "mdns_spectra_set_counts", "with variances")
    assert hip.mdns_spectra_counts(muse.handle) == 0
    refused(hip.mdns_curve_poisson_batch(muse.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(got)),
             "mdns_curve_poisson_batch", "spectra are not in counts mode (mdns_spectra_set_counts)")
    muse.close()
    # a bad exposure is found in the host array, named, and nothing is uploaded: the handle scores as before
    plain = GaussLineSpectra(d["x"], st.y, noise_level=1.0)
    before = plain.loglike_batch_curves(curves)
    for bad in (-1.0, np.nan, np.inf):
        wrong = rows.copy()
        wrong[7, 5] = bad
        refused(hip.mdns_spectra_set_counts(plain.handle, _lib.ptr(wrong), None), "mdns_spectra_set_counts", "exposure[7][5]")
        assert hip.mdns_spectra_counts(plain.handle) == 0
    refused(hip.mdns_curve_poisson_batch(plain.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(got)), "not in counts mode")
    d_c, d_o = hip.mdns_dev_alloc(curves.nbytes), hip.mdns_dev_alloc(got.nbytes)
    refused(hip.mdns_curve_poisson_batch_dev(plain.handle, d_c, nx, 5, None, ndata, d_o), "mdns_curve_poisson_batch_dev", "not in counts mode")
    assert np.array_equal(plain.loglike_batch_curves(curves), before)
    # once a joint state exists on the handle
    js = jointstate.CurveJointState(plain, 8, line_model(d["x"]))
    refused(hip.mdns_spectra_set_counts(plain.handle, _lib.ptr(rows), None), "mdns_spectra_set_counts", "a joint state exists")
    assert hip.mdns_spectra_counts(plain.handle) == 0
    js.close()
    assert np.array_equal(plain.loglike_batch_curves(curves), before)
    # now it goes through; the other setters refuse as on any handle without variances, and the mode stays
    K = np.ascontiguousarray(st.K)
    assert hip.mdns_spectra_set_counts(plain.handle, _lib.ptr(rows), _lib.ptr(K)) == 0 and hip.mdns_spectra_counts(plain.handle) == 1
    refused(hip.mdns_spectra_set_fixed_scale(plain.handle, 1), "mdns_spectra_set_fixed_scale", "without variances")
    refused(hip.mdns_spectra_set_continuum(plain.handle, 2), "mdns_spectra_set_continuum", "variances")
    assert hip.mdns_spectra_counts(plain.handle) == 1 and hip.mdns_spectra_fixed_scale(plain.handle) == 0
    assert hip.mdns_curve_poisson_batch(plain.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(got)) == 0
    counts = CountSpectra(d["x"], d["y"], d["e"])
    assert np.array_equal(got, counts.loglike_batch_curves(curves))
    # the Gaussian batch functions keep computing what their names say (the y on the handle: st.y, masked already)
    assert np.array_equal(plain.loglike_batch_curves(curves), before)
    js = jointstate.CurveJointState(counts, 8, count_model(d["x"]))
    refused(hip.mdns_spectra_set_counts(counts.handle, None, None), "mdns_spectra_set_counts", "a joint state exists")
    js.close()
    # sizes, as mdns_curve_chi2_batch[_dev]
    refused(hip.mdns_curve_poisson_batch(counts.handle, _lib.ptr(curves), 5, None, ndata + 1, _lib.ptr(got)), "mdns_curve_poisson_batch", "M=%d" % (ndata + 1))
    refused(hip.mdns_curve_poisson_batch_dev(counts.handle, d_c, nx - 1, 5, None, ndata, d_o), "mdns_curve_poisson_batch_dev", "ldc=%d" % (nx - 1), "nx=%d" % nx)
    refused(hip.mdns_curve_poisson_batch_dev(counts.handle, None, nx, 5, None, ndata, d_o), "mdns_curve_poisson_batch_dev", "null argument")
    assert hip.mdns_curve_poisson_batch_dev(counts.handle, d_c, nx, 0, None, ndata, d_o) == 0
    assert hip.mdns_curve_poisson_batch_dev(counts.handle, d_c, nx, 5, None, 0, d_o) == 0
    assert np.array_equal(got, counts.loglike_batch_curves(curves))
    hip.mdns_dev_free(d_c)
    hip.mdns_dev_free(d_o)
    # the class passes a bad exposure on as ValueError before any device call
    with pytest.raises(ValueError):
        CountSpectra(d["x"], st.y, -st.e)
    plain.close()
    counts.close()


def test_a_counts_state_takes_curve_chunks_only(hip):
    ndata, nlive, nx = 20, 8, 64
    d = count_data(ndata, nx, seed=11, edges=False)
    spectra = CountSpectra(d["x"], d["y"], d["e"])
    model = count_model(d["x"])
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(DeviceScorer(spectra), nlive, ndata, model)
    rng = np.random.RandomState(3)
    rows5 = np.ones((nlive, 5))
    only = "counts spectra take curve chunks only"
    refused(hip.mdns_joint_init_muse3(dev._h, _lib.ptr(rows5), None), "mdns_joint_init_muse3", only)
    refused(hip.mdns_joint_init_gauss(dev._h, _lib.ptr(rows5), 1.0), "mdns_joint_init_gauss", only)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    dev.init(xs0)
    host.init(xs0)
    dev.prepare()
    host.prepare()
    accepted, nscored, npairs = C.c_int(7), C.c_int(0), C.c_int(0)
    bits = np.zeros(1, dtype=np.uint64)
    assert hip.mdns_backend_draw_begin(dev._h, None, ndata) == 0
    refused(hip.mdns_backend_draw_chunk(dev._h, _lib.ptr(rows5), 4, None, C.addressof(accepted), _lib.ptr(bits), C.addressof(nscored)),
             "mdns_backend_draw_chunk", only)
    assert accepted.value == -1
    refused(hip.mdns_backend_draw_score(dev._h, _lib.ptr(rows5), 4, None), "mdns_backend_draw_score", only)
    bound = np.zeros(4)
    status, pb, pk = (np.zeros(64, dtype=np.int32) for _ in range(3))
    pL, pt = np.zeros(64), np.zeros(64)
    refused(hip.mdns_backend_draw_band_begin(dev._h, _lib.ptr(rows5), 4, _lib.ptr(bound)), "mdns_backend_draw_band", only)
    refused(hip.mdns_backend_draw_band(dev._h, _lib.ptr(rows5), 4, _lib.ptr(bound), _lib.ptr(status), C.addressof(npairs), _lib.ptr(pb),
                                        _lib.ptr(pk), _lib.ptr(pL), _lib.ptr(pt), 64), "mdns_backend_draw_band", only)
    d_p = hip.mdns_dev_alloc(rows5.nbytes)
    refused(hip.mdns_joint_score_dev(dev._h, d_p, 4, 1.0, None, ndata), "mdns_joint_score_dev", only)
    hip.mdns_dev_free(d_p)
    # ... and the state goes on as if nothing had happened: curve chunks decide as the statement does
    for attempt in range(6):
        cube = rng.uniform(size=(9, 3))
        cube[:, 0] *= 0.05
        xs = gauss_prior(cube)
        sel = None if attempt % 2 == 0 else np.arange(attempt % 3, ndata, 3)
        ia, _, ba, na = dev.draw(xs, sel)
        ib, _, bb, _ = host.draw(xs[:na], sel)
        assert ia == ib and (ia < 0 or np.array_equal(ba, bb)), attempt
        ha, hn = dev.thresholds()
        hb, hm = host.thresholds()
        assert np.array_equal(hn, hm) and np.array_equal(ha, hb)
    dev.close()
    spectra.close()


def test_a_handle_without_the_mode_scores_as_before(hip):
    """mdns_curve_loglike_batch on one handle, before and after a DIFFERENT handle was put into counts mode and used."""
    nx, ndata, B = 65, 130, 33
    d = count_data(ndata, nx, seed=12, edges=False)
    y = np.where(np.isfinite(d["y"]), d["y"], 0.0)
    curves = _curves(B, nx, 12)
    plain = GaussLineSpectra(d["x"], y, noise_level=0.5)
    sel = np.arange(1, ndata, 2)
    before = [plain.loglike_batch_curves(curves, rows) for rows in (None, sel)]
    params = gauss_prior(np.random.RandomState(12).uniform(size=(7, 3)))
    params[:, 2] = 10 ** params[:, 2]
    before_k1 = plain.loglike_batch(params)
    counts = CountSpectra(d["x"], y, d["e"])
    assert np.isfinite(counts.loglike_batch_curves(curves)).all()
    assert hip.mdns_spectra_counts(plain.handle) == 0 and hip.mdns_spectra_counts(counts.handle) == 1
    after = [plain.loglike_batch_curves(curves, rows) for rows in (None, sel)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(plain.loglike_batch(params), before_k1)
    counts.close()
    plain.close()
