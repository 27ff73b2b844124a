"""The W statistic of count spectra with a background on the GPU (csrc/mdns_curves.hip k_curve_rows_b and
k_curve_background, include/mdns.h Part 11): the kernel against the longdouble statement within the derived bound, the
fitted background rates against the longdouble ones and against the rate the scoring kernel used, the one value of a
(curve, spectrum) pair, the masked, zero and invalid rules to the bit, the joint state and a whole run against their
numpy statements over the same scores, what is refused, and that a handle without the mode scores as before."""
import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, _Spectra
from curves_support import Chunks, StatementProblem, dev_batch, gauss_prior, refused, selections
from filter_support import _drive
from poisson_support import NumpyPoisson
from wstat_support import DeviceScorer, NumpyWstat, rate, rate_within_bound, source_model, within_bound, wstat_data

pytestmark = pytest.mark.gpu

NX = (1, 2, 15, 16, 17, 33, 64, 513)
BS = (1, 8, 9, 32, 33, 70)
MS = (1, 64, 65, 128, 129)
# (nx, ndata, B, exposures given): every nx, every B, ndata up to 300 -- the cases with 300 spectra carry the sparse
# selections of MS --, paired so that the longdouble reference of a case stays below a million (pair, channel)s
CASES = [(1, 300, 70, True), (2, 70, 33, False), (15, 300, 32, True), (16, 3, 9, False), (17, 300, 8, False),
         (33, 70, 70, True), (64, 300, 33, False), (513, 70, 9, True), (513, 300, 1, False), (64, 1, 1, True),
         (16, 300, 70, True)]


def test_the_cases_cover_every_size():
    assert {c[0] for c in CASES} == set(NX) and {c[2] for c in CASES} == set(BS) and max(c[1] for c in CASES) == 300
    assert {c[3] for c in CASES} == {True, False} and sum(1 for c in CASES if c[1] == 300) >= 4
    assert max(c[0] * c[1] * c[2] for c in CASES) < 1e6


def _curves(B, nx, seed, st=None):
    """Source rates between 0.01 and 1e4 with a few exact zeros (of either sign); with a statement, every fourth curve
    follows N / T of one spectrum to a relative 1e-9: T c' ~ N, where the two branches of f meet."""
    rng = np.random.RandomState(seed)
    curves = 10 ** rng.uniform(-2, 4, size=(B, nx))
    if st is not None:
        for b in range(0, B, 4):
            k = rng.randint(st.ndata)
            T, N = st.e[:, k] + st.g[:, k], st.y[:, k] + st.b[:, k]
            curves[b] = np.where(T > 0, N / np.where(T > 0, T, 1.0), 1.0) * (1 + 1e-9 * rng.normal(size=nx))
    curves[rng.uniform(size=curves.shape) < 0.02] = 0.0
    curves[rng.uniform(size=curves.shape) < 0.01] = -0.0
    return curves


def _t(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=float).T)


class _RawBackground(_Spectra):
    """A handle given counts mode and a background through the raw ABI: ``y``, ``e``, ``b``, ``g`` [nx, ndata] as they
    are (e, g None: NULL), ``offsets`` or NULL for both."""

    def __init__(self, x, y, e, b, g, K=None, Kw=None):
        super(_RawBackground, self).__init__(x, y, None)
        e, b, g = _t(e), _t(b), _t(g)
        K, Kw = (None if a is None else np.ascontiguousarray(a, dtype=float) for a in (K, Kw))
        opt = lambda a: _lib.ptr(a) if a is not None else None
        _lib.check(self._lib.mdns_spectra_set_counts(self._h, opt(e), opt(K)), "mdns_spectra_set_counts")
        _lib.check(self._lib.mdns_spectra_set_background(self._h, opt(b), opt(g), opt(Kw)), "mdns_spectra_set_background")

    def wstat(self, curves, rows=None):
        return self._batch(self._lib.mdns_curve_wstat_batch, "mdns_curve_wstat_batch", np.atleast_2d(_lib.as_f64(curves)), rows)

    def poisson(self, curves, rows=None):
        return self._batch(self._lib.mdns_curve_poisson_batch, "mdns_curve_poisson_batch", np.atleast_2d(_lib.as_f64(curves)), rows)


@pytest.mark.parametrize("nx,ndata,B,exposure", CASES)
def test_kernel_against_the_statement(nx, ndata, B, exposure, hip):
    """Every L within ``bound`` of the longdouble statement (wstat_support derives it), over the whole set and over
    sparse selections of 1, 64, 65, 128 and 129 spectra, both entry points the same bits; backgrounds from 0.05 to 50
    counts per pixel, planted g = 0, NaN counts, an all-zero and a fully masked spectrum; curves from 0 to 1e4 in which
    both branches of f and T c' ~ N occur."""
    rng = np.random.RandomState(nx * 1000 + B)
    d = wstat_data(ndata, nx, seed=2, exposure=exposure)
    st = NumpyWstat(d["y"], d["e"], d["b"], d["g"])
    spectra = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    assert hip.mdns_spectra_counts(spectra.handle) == 1 and hip.mdns_spectra_background(spectra.handle) == 1
    assert np.array_equal(spectra.n_masked, st.n_masked) and spectra.continuum == 0 and spectra.has_background
    curves = _curves(B, nx, nx + B, st)
    up, down, near = st.branches(curves)
    if nx * ndata * B >= 1000:
        assert up > 0.02 and down > 0.02 and near > 0, (up, down, near)
    want = (st.loglike_batch_long(curves),) + st.sums_long(curves)        # once, for every selection
    worst = 0.0
    for name, rows in selections(ndata, rng, MS):
        got = spectra.loglike_batch_curves(curves, rows)
        assert got.shape == (B, ndata if rows is None else len(rows))
        ok, frac = within_bound(got, st, nx, curves, rows, want)
        worst = max(worst, frac)
        assert ok, (name, frac)
        assert np.array_equal(dev_batch(hip, spectra, curves, 3, rows, "mdns_curve_wstat_batch_dev"), got), name
        assert np.array_equal(spectra.loglike_batch(curves, rows), got), name
    print("nx=%d ndata=%d B=%d exposure=%s: worst error %.3g of the bound; a >= 0 in %.2f, a < 0 in %.2f, %d near" %
          (nx, ndata, B, exposure, worst, up, down, near))
    if ndata >= 3:
        whole = spectra.loglike_batch_curves(curves)
        gone = 2 * ndata // 3
        assert st.n_masked[gone] == nx and (whole[:, gone] == 0).all() and not np.signbit(whole[:, gone]).any()
    spectra.close()


@pytest.mark.parametrize("nx,ndata,B,exposure", [(33, 70, 9, True), (17, 300, 8, False), (513, 3, 2, True)])
def test_background_fit_against_the_statement(nx, ndata, B, exposure, hip):
    """f [B, M, nx] within its part of the bound -- FU u (c' + f + N / T) -- of the longdouble f, 0 at a masked pixel,
    over full and sparse selections and both entry points; and a sample of 2000 pixels bit-equal to the float64
    emulation of the chain's operations with a correctly rounded sqrt and / (IEEE arithmetic has one answer: this is
    where the assumption of wstat_support about the device's sqrt and / is checked)."""
    rng = np.random.RandomState(nx + B)
    d = wstat_data(ndata, nx, seed=3, exposure=exposure)
    st = NumpyWstat(d["y"], d["e"], d["b"], d["g"])
    spectra = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    curves = _curves(B, nx, nx + B, st)
    worst = 0.0
    for name, rows in selections(ndata, rng, MS):
        f = spectra.background_fit(curves, rows)
        assert f.shape == (B, ndata if rows is None else len(rows), nx)
        ok, frac = rate_within_bound(f, st, curves, rows)
        worst = max(worst, frac)
        assert ok, (name, frac)
        assert np.array_equal(dev_batch(hip, spectra, curves, 5, rows, "mdns_curve_background_batch_dev", per=nx), f), name
    f = spectra.background_fit(curves)
    assert (f[:, st.masked.T] == 0).all() and (f >= 0).all()
    pick = [(rng.randint(B), rng.randint(ndata), rng.randint(nx)) for _ in range(2000)]
    same = sum(f[b, k, j] == rate(abs(float(curves[b, j])), *(float(a[j, k]) for a in (st.y, st.e, st.b, st.g))) for b, k, j in pick)
    print("nx=%d ndata=%d B=%d: f at %.3g of its bound; %d of 2000 bit-equal to the correctly rounded emulation" % (nx, ndata, B, worst, same))
    assert same == 2000
    spectra.close()


def test_background_fit_is_the_rate_the_scoring_kernel_used(hip):
    """k_curve_rows_b and k_curve_background call the same two device functions (wstat_pixel, wstat_rate) on the same
    operands, and the translation unit holds no expression a compiler may contract: the bits are the same by
    construction.  Where the kernel's score can be solved for f exactly it is checked: one-channel spectra with n = 1,
    b = 0, e = 2**-1000, g = 1 and no offsets have T = 1, a = 1 - c', f = a for c' < 1; where s = c' + f comes out as 1
    exactly, log(s) = 0 and the chain is fma(-1, f, fma(-2**-1000, 1, +0)) = -f.  And a NaN along an invalid value."""
    M = 40
    c = np.arange(1, M + 1) / 64.0                                        # 1 - c' is exact, c' + (1 - c') = 1
    ones = np.ones((1, M))
    probe = _RawBackground(np.zeros(1), ones, 2.0 ** -1000 * ones, 0 * ones, ones)
    L = probe.wstat(c[:, None])
    f = np.empty((M, M, 1))
    _lib.check(hip.mdns_curve_background_batch(probe.handle, _lib.ptr(np.ascontiguousarray(c[:, None])), M, None, M, _lib.ptr(f)),
               "mdns_curve_background_batch")
    assert np.array_equal(f[:, :, 0], np.broadcast_to((1 - c)[:, None], (M, M))) and np.array_equal(L, -f[:, :, 0])
    bad = np.array([[-1.0], [0.5], [np.nan]])
    fb = np.empty((3, M, 1))
    _lib.check(hip.mdns_curve_background_batch(probe.handle, _lib.ptr(bad), 3, None, M, _lib.ptr(fb)), "mdns_curve_background_batch")
    assert np.isnan(fb[0]).all() and np.isnan(fb[2]).all() and (fb[1] == 0.5).all()
    probe.close()


def test_a_pair_has_one_value(hip):
    """The same bits for (curve b, spectrum k) in a batch of 1024 x 130, alone, in a permuted batch over a sparse
    selection, through the device entry with another row stride, and in the live matrix of a joint state."""
    rng = np.random.RandomState(11)
    nx, ndata, B = 33, 130, 1024
    d = wstat_data(ndata, nx, seed=4)
    st = NumpyWstat(d["y"], d["e"], d["b"], d["g"])
    curves = _curves(B, nx, 4, st)
    spectra = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    whole = spectra.loglike_batch_curves(curves)
    assert np.isfinite(whole).all()
    for b, k in [(0, 0), (1023, 129), (3, 63), (4, 64), (5, 127), (1020, 128), (7, 65), (513, 1)]:
        alone = spectra.loglike_batch_curves(curves[b:b + 1], np.array([k]))
        assert alone.shape == (1, 1) and np.array_equal(alone[0, 0], whole[b, k]), (b, k)
    perm = rng.permutation(B)
    sel = np.sort(rng.choice(ndata, size=67, replace=False))
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm], sel), whole[perm][:, sel])
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm[:5]], sel[3:4]), whole[perm[:5]][:, sel[3:4]])
    for pad in (0, 1, 56):
        assert np.array_equal(dev_batch(hip, spectra, curves[perm[:70]], pad, sel, "mdns_curve_wstat_batch_dev"), whole[perm[:70]][:, sel]), pad
    nlive = 40
    js = jointstate.CurveJointState(spectra, nlive, lambda xs: curves[xs[:, 0].astype(int)])
    js.init(np.arange(20, 20 + nlive, dtype=float)[:, None])
    assert np.array_equal(js.live_matrix(), whole[20:20 + nlive])
    js.close()
    spectra.close()


@pytest.mark.parametrize("side", ["source", "background"])
@pytest.mark.parametrize("name,bad", [("first", [0]), ("last", [47]), ("stage", list(range(16, 32))), ("scattered", [1, 15, 16, 32, 46]),
                                      ("all but one", [j for j in range(48) if j != 20])])
def test_a_masked_pixel_is_a_deleted_channel(name, bad, side):
    """e = 0 (or NaN, or a NaN count) -- or, ``background``, g = 0 (or NaN, or a NaN background count) and nothing else
    -- in some channels of every spectrum: the bits of the same data with those channels deleted, whatever the curve
    says there; and the fitted rate is 0 there."""
    nx, ndata, B = 48, 70, 9
    d = wstat_data(ndata, nx, seed=6, edges=False)
    curves = _curves(B, nx, 6)
    arrays = {k: d[k].copy() for k in ("y", "e", "b", "g")}
    exposure, counts = ("e", "y") if side == "source" else ("g", "b")
    arrays[exposure][bad[0::3]] = 0.0
    arrays[exposure][bad[1::3]] = np.nan
    arrays[counts][bad[2::3]] = np.nan
    keep = np.setdiff1d(np.arange(nx), bad)
    with_mask = CountSpectra(d["x"], arrays["y"], arrays["e"], arrays["b"], arrays["g"])
    deleted = CountSpectra(d["x"][keep], *(np.ascontiguousarray(d[k][keep]) for k in ("y", "e", "b", "g")))
    assert (with_mask.n_masked - deleted.n_masked == len(bad)).all()
    wild = curves.copy()
    wild[:, bad] = 10 ** np.random.RandomState(7).uniform(-300, 300, size=(B, len(bad)))
    a = with_mask.loglike_batch_curves(curves)
    assert np.array_equal(a, deleted.loglike_batch_curves(np.ascontiguousarray(curves[:, keep]))) and np.isfinite(a).all()
    assert np.array_equal(a, with_mask.loglike_batch_curves(wild))
    f = with_mask.background_fit(wild)
    assert (f[:, :, bad] == 0).all() and np.array_equal(f[:, :, keep], deleted.background_fit(np.ascontiguousarray(curves[:, keep])))
    with_mask.close()
    deleted.close()


def test_the_edges_to_the_bit(hip):
    """The fully masked spectrum scores +0.0; the all-zero one what the C statistic's kernel gives it (f = 0: -sum e c);
    c = 0 (either sign) where n = b = 0 adds nothing; c = +-0 where n > 0, b = 0 costs no penalty; a negative and a NaN
    curve value NaN for every selected spectrum and for no other candidate of the batch."""
    nx, ndata, B = 33, 70, 9
    d = wstat_data(ndata, nx, seed=8)
    st = NumpyWstat(d["y"], d["e"], d["b"], d["g"])
    spectra = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    zero, gone = ndata // 3, 2 * ndata // 3
    assert spectra.n_masked[gone] == nx and st.Kw[gone] == 0 and st.Kw[zero] == 0 and not st.y[:, zero].any() and not st.b[:, zero].any()
    curves = _curves(B, nx, 8, st)
    L = spectra.loglike_batch_curves(curves)
    assert (L[:, gone] == 0).all() and not np.signbit(L[:, gone]).any()
    plain = CountSpectra(d["x"], st.y, st.e)
    assert np.array_equal(L[:, zero], plain.loglike_batch_curves(curves)[:, zero]) and (L[:, zero] < 0).all()
    plain.close()
    # the zero model: a probe of four channels, n = (0, 3, 0, 2), b = (0, 1, 0, 0), e = (1, 2, 0.5, 1.5), g = (2, 2, 1, 3)
    col = lambda *v: np.array(v, dtype=float)[:, None]
    n, b, e, g = col(0, 3, 0, 2), col(0, 1, 0, 0), col(1, 2, 0.5, 1.5), col(2, 2, 1, 3)
    probe = _RawBackground(np.arange(4.0), n, e, b, g)
    short = _RawBackground(np.arange(2.0), n[[1, 3]], e[[1, 3]], b[[1, 3]], g[[1, 3]])
    c = np.array([[0.0, 0.25, -0.0, 1.0],           # c = +-0 where n = b = 0: nothing
                  [0.25, 0.5, 1.0, 0.0],            # c = +0 where n = 2, b = 0
                  [0.25, 0.5, 1.0, -0.0]])          # c = -0 there
    Lp = probe.wstat(c)[:, 0]
    assert Lp[0] == short.wstat(c[:1, [1, 3]])[0, 0]
    assert Lp[1] == Lp[2] and np.isfinite(Lp).all()
    fp = np.empty((3, 1, 4))
    _lib.check(hip.mdns_curve_background_batch(probe.handle, _lib.ptr(c), 3, None, 1, _lib.ptr(fp)), "mdns_curve_background_batch")
    assert fp[1, 0, 3] == 2 / 4.5 and fp[2, 0, 3] == 2 / 4.5 and (fp[0, 0, [0, 2]] == 0).all()
    # (n = 2 at f = n / T: 2 log(2 / 4.5) - 1.5 f - 3 f = 2 log(2 / 4.5) - 2, no -708 per count)
    assert abs((Lp[1] - probe.wstat(np.array([[0.25, 0.5, 1.0, 1e-300]]))[0, 0])) < 1e-12 and Lp[1] > -20
    probe.close()
    short.close()
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
    """mdns_spectra_set_background through the raw ABI: NULL exposures are ones, NULL offsets zeros, and all four values
    are zeroed where either side is masked (counts still in place under e = 0 or g = 0: the library zeroes them)."""
    nx, ndata, B = 31, 70, 8
    d = wstat_data(ndata, nx, seed=9)
    st = NumpyWstat(d["y"], d["e"], d["b"], d["g"])
    y, b = np.where(st.masked, 3.0, st.y), np.where(st.masked, 2.0, st.b)
    e, g = st.e.copy(), st.g.copy()
    half = st.masked & (np.arange(nx)[:, None] % 2 == 0)
    e[half], g[st.masked & ~half] = 1.5, 2.5                             # (masked on ONE side only, counts on both)
    assert np.array_equal(NumpyWstat(y, e, b, g).masked, st.masked)
    curves = _curves(B, nx, 9, st)
    cls = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    raw = _RawBackground(d["x"], y, e, b, g, None, st.Kw)
    assert np.array_equal(raw.wstat(curves), cls.loglike_batch_curves(curves))
    no_k = _RawBackground(d["x"], y, e, b, g)
    assert np.array_equal(no_k.wstat(curves) + st.Kw[None, :], raw.wstat(curves))
    yy, bb = np.where(np.isfinite(d["y"]), d["y"], 0.0), np.where(np.isfinite(d["b"]), d["b"], 0.0)
    ones = _RawBackground(d["x"], yy, None, bb, None)
    given = _RawBackground(d["x"], yy, np.ones_like(yy), bb, np.ones_like(yy), np.zeros(ndata), np.zeros(ndata))
    assert np.array_equal(ones.wstat(curves), given.wstat(curves))
    st1 = NumpyWstat(yy, None, bb, None)
    ok, frac = within_bound(ones.wstat(curves) + st1.Kw[None, :], st1, nx, curves)
    assert ok, frac
    for s in (cls, raw, no_k, ones, given):
        s.close()


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("ndata,nlive,nx", [(20, 8, 64), (130, 12, 33)])
def test_joint_state_equals_its_numpy_statement(ndata, nlive, nx, noisy):
    """CurveJointState over CountSpectra with a background against HostJointState fed by mdns_curve_wstat_batch: accepted
    index, fill bits, thresholds and live matrix equal, over several prepare / draw / advance rounds, with and without
    jitter."""
    rng = np.random.RandomState(ndata * 7 + nlive + noisy)
    d = wstat_data(ndata, nx, seed=8, edges=False)
    spectra = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    model = source_model(d["x"])
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(DeviceScorer(spectra), nlive, ndata, model)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    noise0 = rng.normal(0, 1e-5, size=(nlive, ndata)) if noisy else None
    dev.init(xs0, jitter=noise0)
    host.init(xs0, jitter=noise0)
    assert dev.nparams == 3 and np.array_equal(dev.live_matrix(), host.live_matrix())
    want = NumpyWstat(d["y"], d["e"], d["b"], d["g"]).loglike_batch_long(model(xs0)).astype(float) + (noise0 if noisy else 0)
    assert np.allclose(dev.live_matrix(), want, rtol=1e-11, atol=1e-9)
    assert _drive(Chunks(dev, lambda xs: xs, noisy), Chunks(host, model, noisy), ndata, rng, iterations=8, exact=True) > 0
    dev.close()
    spectra.close()


def test_whole_run_equals_the_statement():
    d = wstat_data(12, 64, seed=9, edges=False)
    model = source_model(d["x"])
    runs = []
    for cls in (problem.CurveProblem, StatementProblem):
        p = cls(d["x"], d["y"], model, gauss_prior, 3, poisson=True, exposure=d["e"], background=d["b"], background_exposure=d["g"])
        assert isinstance(p.backend, CountSpectra) and p.backend.has_background
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=20, max_samples=40, use_graph=False, seed=1)
        assert type(sampler.joint).__name__ == ("CurveJointState" if cls is problem.CurveProblem else "HostJointState")
        assert sampler.native is not None
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert runs[0][2] > 0 and runs[0][2] == runs[1][2] and np.isfinite(runs[0][0]).all()
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_the_background_is_set_only_where_it_has_a_meaning(hip):
    """Every refusal of include/mdns.h Part 11 names its function and reason and leaves the handle as it was."""
    nx, ndata = 64, 20
    d = wstat_data(ndata, nx, seed=10, edges=False)
    st = NumpyWstat(d["y"], d["e"], d["b"], d["g"])
    b_rows, g_rows = _t(st.b), _t(st.g)
    curves = _curves(5, nx, 10, st)
    got = np.empty((5, ndata))
    fout = np.empty((5, ndata, nx))
    assert hip.mdns_spectra_background(None) == -1
    refused(hip.mdns_spectra_set_background(None, _lib.ptr(b_rows), None, None), "mdns_spectra_set_background", "null")
    # a handle that is not in counts mode
    plain = GaussLineSpectra(d["x"], st.y, noise_level=1.0)
    before = plain.loglike_batch_curves(curves)
    refused(hip.mdns_spectra_set_background(plain.handle, _lib.ptr(b_rows), _lib.ptr(g_rows), None), "mdns_spectra_set_background", "not in counts mode")
    assert hip.mdns_spectra_background(plain.handle) == 0 and np.array_equal(plain.loglike_batch_curves(curves), before)
    plain.close()
    # a counts handle without a background: the new batch functions refuse, the Poisson one goes on
    K0 = NumpyPoisson(d["y"], d["e"]).K                                   # (what CountSpectra gives set_counts below)
    counts = CountSpectra(d["x"], d["y"], d["e"])
    c_before = counts.loglike_batch_curves(curves)
    d_c, d_o = hip.mdns_dev_alloc(curves.nbytes), hip.mdns_dev_alloc(fout.nbytes)
    no = "spectra have no background (mdns_spectra_set_background)"
    refused(hip.mdns_curve_wstat_batch(counts.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(got)), "mdns_curve_wstat_batch", no)
    refused(hip.mdns_curve_wstat_batch_dev(counts.handle, d_c, nx, 5, None, ndata, d_o), "mdns_curve_wstat_batch_dev", no)
    refused(hip.mdns_curve_background_batch(counts.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(fout)), "mdns_curve_background_batch", no)
    refused(hip.mdns_curve_background_batch_dev(counts.handle, d_c, nx, 5, None, ndata, d_o), "mdns_curve_background_batch_dev", no)
    with pytest.raises(ValueError):
        counts.background_fit(curves)
    # null counts; a bad exposure or count is found in the host arrays, named, and nothing is uploaded
    refused(hip.mdns_spectra_set_background(counts.handle, None, _lib.ptr(g_rows), None), "mdns_spectra_set_background", "null background counts")
    for bad in (-1.0, np.inf, -np.inf):
        wrong = g_rows.copy()
        wrong[7, 5] = bad
        refused(hip.mdns_spectra_set_background(counts.handle, _lib.ptr(b_rows), _lib.ptr(wrong), None), "mdns_spectra_set_background", "bkg_exposure[7][5]")
    wrong = b_rows.copy()
    wrong[3, 9], g_ok = -2.0, g_rows.copy()
    g_ok[3, 9] = 1.0
    refused(hip.mdns_spectra_set_background(counts.handle, _lib.ptr(wrong), _lib.ptr(g_ok), None), "mdns_spectra_set_background", "bkg_counts[3][9]")
    assert hip.mdns_spectra_background(counts.handle) == 0 and np.array_equal(counts.loglike_batch_curves(curves), c_before)
    # once a joint state exists on the handle
    js = jointstate.CurveJointState(counts, 8, source_model(d["x"], floor=0.05))
    refused(hip.mdns_spectra_set_background(counts.handle, _lib.ptr(b_rows), _lib.ptr(g_rows), None), "mdns_spectra_set_background", "a joint state exists")
    js.close()
    assert hip.mdns_spectra_background(counts.handle) == 0 and np.array_equal(counts.loglike_batch_curves(curves), c_before)
    # now it goes through (a NaN exposure masks); set_counts is refused from here on, and the state stays
    g_nan = g_rows.copy()
    g_nan[st.masked.T & (g_rows == 0)] = np.nan
    Kw = np.ascontiguousarray(st.Kw)
    assert hip.mdns_spectra_set_background(counts.handle, _lib.ptr(b_rows), _lib.ptr(g_nan), _lib.ptr(Kw)) == 0
    assert hip.mdns_spectra_background(counts.handle) == 1 and hip.mdns_spectra_counts(counts.handle) == 1
    both = CountSpectra(d["x"], d["y"], d["e"], d["b"], d["g"])
    assert hip.mdns_curve_wstat_batch(counts.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(got)) == 0
    assert np.array_equal(got, both.loglike_batch_curves(curves))
    refused(hip.mdns_spectra_set_counts(counts.handle, None, None), "mdns_spectra_set_counts", "have a background")
    assert np.array_equal(got, both.loglike_batch_curves(curves))
    # mdns_curve_poisson_batch on such a handle: the C statistic of the n, e and K that are on it -- n and e masked
    # under the new rule, K the one given to set_counts
    masked_counts = CountSpectra(d["x"], st.y, st.e)
    k_now = NumpyPoisson(st.y, st.e).K
    pois = np.empty((5, ndata))
    assert hip.mdns_curve_poisson_batch(counts.handle, _lib.ptr(curves), 5, None, ndata, _lib.ptr(pois)) == 0
    assert np.allclose(pois - K0[None, :], masked_counts.loglike_batch_curves(curves) - k_now[None, :], rtol=1e-13, atol=1e-10)
    assert np.array_equal(both._batch(hip.mdns_curve_poisson_batch, "mdns_curve_poisson_batch", curves, None), masked_counts.loglike_batch_curves(curves))
    # sizes and null arguments, as mdns_curve_poisson_batch[_dev]
    refused(hip.mdns_curve_wstat_batch(both.handle, _lib.ptr(curves), 5, None, ndata + 1, _lib.ptr(got)), "mdns_curve_wstat_batch", "M=%d" % (ndata + 1))
    refused(hip.mdns_curve_wstat_batch_dev(both.handle, d_c, nx - 1, 5, None, ndata, d_o), "mdns_curve_wstat_batch_dev", "ldc=%d" % (nx - 1), "nx=%d" % nx)
    refused(hip.mdns_curve_wstat_batch_dev(both.handle, None, nx, 5, None, ndata, d_o), "mdns_curve_wstat_batch_dev", "null argument")
    refused(hip.mdns_curve_background_batch_dev(both.handle, d_c, nx, 5, None, ndata, None), "mdns_curve_background_batch_dev", "null argument")
    assert hip.mdns_curve_wstat_batch_dev(both.handle, d_c, nx, 0, None, ndata, d_o) == 0
    assert hip.mdns_curve_background_batch_dev(both.handle, d_c, nx, 5, None, 0, d_o) == 0
    bad_rows = np.array([0, ndata], dtype=np.int32)
    refused(hip.mdns_curve_background_batch(both.handle, _lib.ptr(curves), 5, _lib.ptr(bad_rows), 2, _lib.ptr(fout)), "mdns_curve_background_batch", "row_ids[1]")
    # a state on a handle with a background refuses set_background too, and takes curve chunks only
    js = jointstate.CurveJointState(both, 8, source_model(d["x"]))
    refused(hip.mdns_spectra_set_background(both.handle, _lib.ptr(b_rows), None, None), "mdns_spectra_set_background", "a joint state exists")
    rows5 = np.ones((8, 5))
    refused(hip.mdns_joint_init_muse3(js._h, _lib.ptr(rows5), None), "mdns_joint_init_muse3", "counts spectra take curve chunks only")
    js.close()
    assert np.array_equal(got, both.loglike_batch_curves(curves))
    hip.mdns_dev_free(d_c)
    hip.mdns_dev_free(d_o)
    # the class passes a bad exposure on as ValueError before any device call
    with pytest.raises(ValueError):
        CountSpectra(d["x"], st.y, st.e, st.b, -st.g)
    for s in (counts, both, masked_counts):
        s.close()


def test_a_handle_without_the_mode_scores_as_before(hip):
    """mdns_curve_poisson_batch on a counts handle and mdns_curve_loglike_batch on a plain one, before and after a
    DIFFERENT handle was given a background and used."""
    nx, ndata, B = 65, 130, 33
    d = wstat_data(ndata, nx, seed=12, edges=False)
    y = np.where(np.isfinite(d["y"]), d["y"], 0.0)
    curves = _curves(B, nx, 12)
    plain = GaussLineSpectra(d["x"], y, noise_level=0.5)
    counts = CountSpectra(d["x"], y, d["e"])
    sel = np.arange(1, ndata, 2)
    before = [s.loglike_batch_curves(curves, rows) for s in (plain, counts) for rows in (None, sel)]
    both = CountSpectra(d["x"], y, d["e"], d["b"], d["g"])
    assert np.isfinite(both.loglike_batch_curves(curves)).all() and np.isfinite(both.background_fit(curves[:2])).all()
    assert hip.mdns_spectra_background(plain.handle) == 0 and hip.mdns_spectra_background(counts.handle) == 0
    assert hip.mdns_spectra_background(both.handle) == 1
    after = [s.loglike_batch_curves(curves, rows) for s in (plain, counts) for rows in (None, sel)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    for s in (plain, counts, both):
        s.close()
