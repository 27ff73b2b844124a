"""The Poisson likelihood of count spectra on the CPU tier: the statement and the emulated chain against the bound the
GPU tests use, L = -C/2, the masking rule of ``like.count_pixels``, the zero and invalid model,
``problem.CurveProblem(poisson=True)`` over the numpy statement, the ``MDNS_MODEL`` switch, and what the likelihood is
for: an amplitude from a handful of counts per pixel, where the Gaussian form with v = max(n, 1) comes out low."""
import numpy as np
import pytest

from massivedatans_amd import constrainer, gen, jointstate, problem, sample
from massivedatans_amd.like import count_pixels
from chi2_support import NumpyWeightedChi2
from curves_support import gauss_prior
from oracle_backend import patch_neighbors
from poisson_support import LOG_ULPS, TINY, NumpyPoisson, _fma, bound, chain, count_data, count_model, within_bound

LOG_TINY = float(np.log(TINY))


def _curves(B, nx, seed):
    """Count rates between 0.01 and 60, with a few exact zeros."""
    rng = np.random.RandomState(seed)
    curves = 10 ** rng.uniform(-2, np.log10(60.0), size=(B, nx))
    curves[rng.uniform(size=curves.shape) < 0.02] = 0.0
    return curves


@pytest.mark.parametrize("exposure", [False, True])
@pytest.mark.parametrize("nx", [1, 2, 33, 64, 200, 513])
def test_emulated_chain_lies_within_the_bound(nx, exposure):
    """The float64 chain the kernel computes, emulated operation by operation with numpy's ``log``, against the
    longdouble statement: within ``bound``, the one the GPU tests hold the kernel to; with exposures and their planted
    zeros (masks) and without."""
    ndata, B = 5, 3
    d = count_data(ndata, nx, seed=1, exposure=exposure)
    st = NumpyPoisson(d["y"], d["e"])
    curves = _curves(B, nx, nx)
    got = np.array([[chain(curves[b], st.y[:, k], st.e[:, k], st.K[k]) for k in range(ndata)] for b in range(B)])
    ok, worst = within_bound(got, st, nx, curves)
    print("nx=%d exposure=%s: emulated chain at %.3g of the bound" % (nx, exposure, worst))
    assert ok, worst
    assert LOG_ULPS == 2 and bound(4096, 1.0, 1.0) < 1e-12                # (relative to S: far below the project's 1e-12)
    # the float64 statement (numpy's own summation order) is another rounding of the same sum
    S, _ = st.sums_long(curves)
    assert (np.abs(st.loglike_batch(curves) - st.loglike_batch_long(curves).astype(float)) <= 1e-12 * S.astype(float)).all()
    # the edge spectra: all zeros scores -sum e c by the chain (K = 0), fully masked +0.0
    zero, gone = ndata // 3, 2 * ndata // 3
    assert st.K[zero] == 0 and st.K[gone] == 0 and st.n_masked[gone] == nx
    assert (got[:, gone] == 0).all() and not np.signbit(got[:, gone]).any()
    for b in range(B):
        acc = 0.0
        for j in range(nx):
            acc = _fma(-float(st.e[j, zero]), float(curves[b, j]), acc)   # (fma(0, lc, acc) = acc: the counts drop out)
        assert got[b, zero] == acc and acc <= 0


def test_L_is_minus_half_the_C_statistic():
    """For c > 0: L = -C/2 with C = 2 sum (mu - n + n log(n / mu)), mu = e c, and L <= 0 -- both up to the bound."""
    nx, ndata, B = 64, 7, 4
    d = count_data(ndata, nx, seed=2)
    st = NumpyPoisson(d["y"], d["e"])
    curves = 10 ** np.random.RandomState(2).uniform(-2, 1.5, size=(B, nx))
    L = st.loglike_batch(curves)
    S, nlc = st.sums_long(curves)
    lim = bound(nx, S.astype(float), nlc.astype(float))
    n, e = st.y.astype(np.longdouble), st.e.astype(np.longdouble)
    for b in range(B):
        mu = e * curves[b].astype(np.longdouble)[:, None]
        seen = n > 0
        term = mu - n + np.where(seen, n * (np.log(np.where(seen, n, 1)) - np.log(np.where(seen & (mu > 0), mu, 1))), 0)
        term = np.where(e > 0, term, 0)                                   # (a masked pixel: n = 0 and e = 0)
        C = 2 * term.sum(axis=0)
        assert (C >= 0).all()
        assert (np.abs(L[b].astype(np.longdouble) + C / 2) <= lim[b]).all()
        assert (L[b] <= lim[b]).all()
    # a perfect model (c = n / e wherever e > 0) scores 0 up to the bound
    k = 0
    perfect = np.where(st.e[:, k] > 0, st.y[:, k] / np.where(st.e[:, k] > 0, st.e[:, k], 1), 1.0)
    Sp, nlcp = st.sums_long(perfect[None], np.array([k]))
    assert abs(st.loglike_batch(perfect[None], np.array([k]))[0, 0]) <= bound(nx, float(Sp[0, 0]), float(nlcp[0, 0]))


def test_masking_rule():
    y = np.array([[1.0, np.nan, 3.0], [np.inf, 5.0, 6.0], [7.0, 0.0, -np.inf]])
    e = np.array([[0.5, 1.0, 0.0], [1.0, np.nan, 2.0], [4.0, 1e-300, 1.0]])
    y0, e0 = y.copy(), e.copy()
    yy, ee, masked, K = count_pixels(y, e)
    assert np.array_equal(y, y0, equal_nan=True) and np.array_equal(e, e0, equal_nan=True)        # copies: the caller's arrays stay
    assert np.array_equal(masked, [[False, True, True], [True, True, False], [False, False, True]])
    assert np.array_equal(yy, [[1.0, 0.0, 0.0], [0.0, 0.0, 6.0], [7.0, 0.0, 0.0]])
    assert np.array_equal(ee, [[0.5, 0.0, 0.0], [0.0, 0.0, 2.0], [4.0, 1e-300, 0.0]])
    # offsets: per spectrum (column) over the pixels with n > 0 and e > 0, in longdouble
    ld = np.longdouble
    want = [ld(1) * (1 + np.log(ld(0.5)) - np.log(ld(1))) + ld(7) * (1 + np.log(ld(4)) - np.log(ld(7))), ld(0),
            ld(6) * (1 + np.log(ld(2)) - np.log(ld(6)))]
    assert K.dtype == np.float64 and np.array_equal(K, np.array(want).astype(np.float64))
    # without exposures: all ones; the other layout sums over the other axis
    y1, e1, m1, K1 = count_pixels(yy)
    assert (e1 == 1).all() and not m1.any() and np.array_equal(y1, yy)
    assert np.array_equal(count_pixels(yy.T, ee.T, axis=1)[3], K)
    for name, arr, bad in (("e", 1, -1.0), ("e", 1, np.inf), ("e", 1, -np.inf), ("y", 0, -2.0)):
        a = [y0.copy(), e0.copy()]
        a[arr][2, 0] = bad
        with pytest.raises(ValueError) as err:
            count_pixels(*a)
        assert "%s[2, 0]" % name in str(err.value), str(err.value)
    with pytest.raises(ValueError):
        count_pixels(y0, e0[:2])
    # a bad value under a pixel that is masked anyway is not looked at
    a, b = y0.copy(), e0.copy()
    a[0, 2] = -5.0                                                        # e = 0 there
    b[0, 1] = -1.0                                                        # y is NaN there
    assert np.array_equal(count_pixels(a, b)[2], masked)
    st = NumpyPoisson(y0, e0)
    assert np.array_equal(st.n_masked, [1, 2, 2])


def test_a_masked_pixel_contributes_nothing_whatever_the_curve_says():
    nx, ndata = 33, 5
    d = count_data(ndata, nx, seed=4)
    d["e"][7] = 0.0                                                      # (every spectrum has a masked pixel)
    st = NumpyPoisson(d["y"], d["e"])
    rng = np.random.RandomState(4)
    a = 10 ** rng.uniform(-2, 1.5, size=nx)
    for k in range(ndata):
        b = np.where(st.masked[:, k], 10 ** rng.uniform(-300, 300, size=nx), a)
        b[np.flatnonzero(st.masked[:, k])[:1]] = 0.0
        assert st.n_masked[k] > 0
        assert chain(a, st.y[:, k], st.e[:, k], st.K[k]) == chain(b, st.y[:, k], st.e[:, k], st.K[k])
        sel = np.array([k])
        assert st.loglike_batch(a[None], sel)[0, 0] == st.loglike_batch(b[None], sel)[0, 0]
        # ... and is a deleted channel, bit for bit
        keep = ~st.masked[:, k]
        assert chain(a, st.y[:, k], st.e[:, k], st.K[k]) == chain(a[keep], st.y[keep, k], st.e[keep, k], st.K[k])


def test_the_zero_and_the_invalid_model():
    e = np.array([[1.0], [2.0], [0.5], [1.5]])
    y = np.array([[0.0], [0.0], [0.0], [0.0]])
    st = NumpyPoisson(y, e)
    # c = 0 (either sign) where n = 0 contributes exactly nothing
    for zero in (0.0, -0.0):
        c = np.array([zero, zero, zero, zero])
        for L in (chain(c, st.y[:, 0], st.e[:, 0], st.K[0]), st.loglike_batch(c[None])[0, 0]):
            assert L == 0 and not np.signbit(L)
        c = np.array([0.25, zero, 3.0, zero])
        assert chain(c, st.y[:, 0], st.e[:, 0], st.K[0]) == chain(c[[0, 2]], st.y[[0, 2], 0], st.e[[0, 2], 0], 0.0) == -(0.25 + 1.5)
    # c = 0 at n = 3 costs exactly 3 log(tiny) against the same curve with that pixel masked (whose K holds no term of it)
    y3 = y.copy()
    y3[1, 0] = 3.0
    seen, gone = NumpyPoisson(y3, e), NumpyPoisson(y3, np.where(y3 > 0, 0.0, e))
    K3 = float(np.longdouble(3) * (1 + np.log(np.longdouble(2)) - np.log(np.longdouble(3))))
    assert seen.K[0] == K3 and gone.K[0] == 0 and gone.n_masked[0] == 1
    c = np.zeros(4)
    for a, b in ((chain(c, seen.y[:, 0], seen.e[:, 0], seen.K[0]), chain(c, gone.y[:, 0], gone.e[:, 0], gone.K[0])),
                 (seen.loglike_batch(c[None])[0, 0], gone.loglike_batch(c[None])[0, 0])):
        assert b == 0 and a - b == 3 * LOG_TINY + K3 and np.isfinite(a) and a < -2100
    # ordered: more violated counts are worse
    y5 = y3.copy()
    y5[2, 0] = 2.0
    assert NumpyPoisson(y5, e).loglike_batch(c[None])[0, 0] < seen.loglike_batch(c[None])[0, 0]
    # a negative or NaN curve value: NaN for every spectrum, masked pixel or not
    d = count_data(5, 33, seed=5)
    st = NumpyPoisson(d["y"], d["e"])
    good = 10 ** np.random.RandomState(5).uniform(-2, 1.5, size=33)
    for bad in (-1e-300, -1.0, -np.inf, np.nan):
        for j in (0, 32, int(np.flatnonzero(st.masked[:, 0])[0])):
            c = good.copy()
            c[j] = bad
            L = st.loglike_batch(np.array([good, c]))
            assert np.isfinite(L[0]).all() and np.isnan(L[1]).all()
            assert all(np.isnan(chain(c, st.y[:, k], st.e[:, k], st.K[k])) for k in range(5))


def _case(ndata=12):
    d = count_data(ndata, 64, seed=3, edges=False)
    return d["x"], d["y"], d["e"]


def test_problem_over_the_statement(oracle, monkeypatch):
    """``poisson=True`` over a numpy backend: the surface of the problem, and a short analysis through the numpy joint
    state that comes out the same twice."""
    patch_neighbors(monkeypatch, oracle)
    x, y, e = _case()
    scorer = NumpyPoisson(y, e)
    p = problem.CurveProblem(x, y, count_model(x), gauss_prior, 3, poisson=True, exposure=e, backend=scorer)
    assert p.poisson is True and p.marginalise_scale is True and p.ndata == 12 and p.continuum == 0 and p.v is None
    assert np.array_equal(p.exposure, e)
    xs = gauss_prior(np.random.RandomState(2).uniform(size=(4, 3)))
    mask = np.arange(12) % 3 != 1
    want = scorer.loglike_batch(count_model(x)(xs), mask)
    assert np.array_equal(p.multi_loglikelihood_batch(xs, mask), want)
    assert np.array_equal(p.multi_loglikelihood(xs[1], mask), want[1])
    runs = []
    for _ in range(2):
        p = problem.CurveProblem(x, y, count_model(x), gauss_prior, 3, poisson=True, exposure=e, backend=NumpyPoisson(y, e))
        sampler = sample.build_sampler(p, nlive_points=20, nsuperset_draws=10, use_graph=False, seed=1, fused=True)
        with np.errstate(all="ignore"):
            results = sample.integrate(sampler, 0.5, 0, 40)
        assert isinstance(sampler.joint, jointstate.HostJointState)
        if constrainer.available():
            assert sampler.native is not None
        assert results["logZ"].shape == (12,) and np.isfinite(results["logZ"]).all() and sampler.ndraws > 0
        runs.append((results["logZ"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])


def test_problem_refuses_what_has_no_meaning():
    x, y, e = _case(4)
    backend = NumpyPoisson(y, e)
    for kw, words in ((dict(poisson=True, v=np.ones_like(y)), ("poisson", "v")),
                      (dict(poisson=True, continuum=2), ("poisson", "continuum")),
                      (dict(poisson=True, marginalise_scale=False), ("poisson", "marginalise_scale")),
                      (dict(exposure=e), ("exposure", "poisson"))):
        with pytest.raises(ValueError) as err:
            problem.CurveProblem(x, y, count_model(x), gauss_prior, 3, backend=backend, **kw)
        assert all(w in str(err.value) for w in words), str(err.value)
    assert problem.CurveProblem(x, y, count_model(x), gauss_prior, 3, backend=backend).poisson is False


def test_default_backend_gets_the_keywords_only_when_set(monkeypatch):
    x, y, e = _case(4)
    made = []

    def backend(x, y, noise_level, v=None, **kw):
        made.append((v is not None, dict(kw)))
        return NumpyPoisson(y, kw.get("exposure"))
    monkeypatch.setattr(problem, "default_backend", backend)
    problem.CurveProblem(x, y, count_model(x), gauss_prior, 3)
    p = problem.CurveProblem(x, y, count_model(x), gauss_prior, 3, poisson=True)
    assert p.exposure is None
    problem.CurveProblem(x, y, count_model(x), gauss_prior, 3, poisson=True, exposure=e)
    assert made[0] == (False, {}) and made[1] == (False, {"poisson": True})
    assert made[2][0] is False and set(made[2][1]) == {"poisson", "exposure"} and made[2][1]["poisson"] is True
    assert np.array_equal(made[2][1]["exposure"], e)


MODEL_FILE = """
import numpy
x = numpy.linspace(400.0, 800.0, 64)
ndim = 3
poisson = True
def priortransform_batch(us):
    us = numpy.asarray(us, dtype=float)
    return numpy.column_stack((10 ** (us[:, 0] * 2 - 2), us[:, 1] * 400 + 400, 10 ** (us[:, 2] * 2)))
def model(xs):
    return numpy.array([0.05 + 40 * A * numpy.exp(-0.5 * ((mu - x) / sig) ** 2) for A, mu, sig in xs]).reshape(len(xs), len(x))
"""


def _write_case(tmp_path, with_v):
    x, y, e = _case(6)
    data = str(tmp_path / "data.npz")
    gen.save(data, dict(x=x, y=y, e=e, v=np.ones_like(y)) if with_v else dict(x=x, y=y, e=e))
    path = tmp_path / "mymodel.py"
    path.write_text(MODEL_FILE)
    return data, str(path)


def test_load_model_returns_the_switch(tmp_path):
    _, path = _write_case(tmp_path, False)
    assert sample.load_model(path)["poisson"] is True
    other = tmp_path / "other.py"
    other.write_text(MODEL_FILE.replace("poisson = True\n", ""))
    assert sample.load_model(str(other))["poisson"] is False


def test_mdns_model_drives_main_with_counts(tmp_path, oracle, monkeypatch, capsys):
    patch_neighbors(monkeypatch, oracle)
    data, path = _write_case(tmp_path, False)
    made = []

    def backend(x, y, noise_level, v=None, **kw):
        made.append((len(x), y.shape, v, kw.get("poisson"), kw["exposure"].shape, sorted(kw)))
        return NumpyPoisson(y, kw["exposure"])
    monkeypatch.setattr(problem, "default_backend", backend)
    monkeypatch.setenv("MDNS_MODEL", path)
    monkeypatch.setenv("NLIVE_POINTS", "20")
    monkeypatch.setenv("MAXSAMPLES", "30")
    monkeypatch.setenv("USE_GRAPH", "0")
    monkeypatch.delenv("MDNS_POSTERIOR", raising=False)
    sample.main(["sample", data, "5"])
    assert made == [(64, (64, 5), None, True, (64, 5), ["exposure", "poisson"])]
    out = capsys.readouterr().out
    assert "logZ = " in out and "ndraws:" in out
    written = gen.read_datasets(data + "_MLFRIENDS_nlive20_5.out8.npz")
    assert written["logZ"].shape == (5,) and np.isfinite(written["logZ"]).all() and int(written["ndraws"]) > 0


def test_mdns_model_with_counts_excludes_variances(tmp_path, monkeypatch):
    data, path = _write_case(tmp_path, True)
    monkeypatch.setenv("MDNS_MODEL", path)
    with pytest.raises(SystemExit) as e:
        sample.main(["sample", data, "6"])
    assert e.value.code not in (0, None) and "poisson" in str(e.value.code) and "`v`" in str(e.value.code)


def test_the_amplitude_comes_out_right_only_with_the_poisson_form():
    """What the likelihood is for.  12 spectra hold the same broad line at 12 amplitudes A = 4.0, 4.5 ... 9.5 counts per
    pixel and unit exposure at the peak -- a few counts per pixel, fewer in the wings, most pixels of the wings empty.
    Over a grid of 9 amplitudes around each truth (centre and width at their true values) the Poisson statement peaks at
    the grid point nearest the truth, for all 12; the Gaussian form with v = max(n, 1) peaks LOW, for all 12.

    The sizing.  With the curve A g_j the Fisher information of A is sum_j e_j g_j / A, so the maximum-likelihood
    amplitude scatters by sigma_A = (A / sum_j e_j g_j)^1/2 around the truth, which is a grid point: the peak is off by
    one when |A^ - A| > step / 2.  4096 channels under a line 600 channels wide give sum e g of about 1900 and
    sigma_A <= 0.072; the grid spacing is 0.8, so that is a 5 sigma event (asserted below from the exposures alone)."""
    ndata, nx, step, half = 12, 4096, 0.8, 4
    x = np.arange(nx, dtype=float)
    g = np.exp(-0.5 * ((x - 2047.3) / 600.0) ** 2)
    rng = np.random.RandomState(12)
    e = rng.uniform(0.5, 2.0, size=(nx, ndata))
    truth = 4.0 + 0.5 * np.arange(ndata)
    y = rng.poisson(e * truth[None, :] * g[:, None]).astype(float)
    sigma_A = np.sqrt(truth / (e * g[:, None]).sum(axis=0))
    assert sigma_A.max() <= 0.072 and step / 2 >= 5 * sigma_A.max() and truth.min() - half * step > 0
    assert np.median(y[np.abs(x - 2047.3) < 300]) <= 9 and (y[np.abs(x - 2047.3) > 1500] == 0).mean() > 0.5
    poisson = NumpyPoisson(y, e)
    # the Gaussian form a user without this likelihood falls back to: counts per unit exposure with v = max(n, 1) / e^2
    gauss = NumpyWeightedChi2(y / e, np.maximum(y, 1.0) / e ** 2)
    for k in range(ndata):
        grid = truth[k] + step * (np.arange(2 * half + 1) - half)
        sel = np.arange(ndata) == k
        curves = grid[:, None] * g[None, :]
        L = poisson.loglike_batch(curves, sel)[:, 0]
        assert int(np.argmax(L)) == half, (k, int(np.argmax(L)))
        assert L[half] - max(L[half - 1], L[half + 1]) > 1.0                # a peak, not a tie
        Lg = gauss.loglike_batch(curves, sel)[:, 0]
        assert int(np.argmax(Lg)) < half, (k, int(np.argmax(Lg)))
