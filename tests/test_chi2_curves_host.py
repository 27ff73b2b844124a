"""The fixed-scale chi^2 with per-pixel variances on the CPU tier: the statement and the emulated chain against the
bound the GPU tests use, the masking rule of ``like.WeightedSpectra``, ``problem.CurveProblem(marginalise_scale=False)``
over the numpy statement, the ``MDNS_MODEL`` switch, and what the likelihood is for: the amplitude of a model."""
import numpy as np
import pytest

from massivedatans_amd import constrainer, gen, jointstate, problem, sample
from massivedatans_amd.like import mask_pixels
from chi2_support import NumpyWeightedChi2, chain, rel_bound, weighted_data
from curves_support import NumpyScaleMarginalised, gauss_prior, line_model
from oracle_backend import patch_neighbors


@pytest.mark.parametrize("nx,masked", [(1, False), (2, False), (33, True), (64, True), (200, False), (513, True)])
def test_emulated_chain_lies_within_the_bound(nx, masked):
    """The float64 chain the kernel computes, emulated operation by operation, against the longdouble statement:
    within (nx + 4) 2^-53, the bound the GPU tests hold the kernel to; and far below the project's 1e-12."""
    ndata, B = 5, 3
    d = weighted_data(ndata, nx, seed=1, masked=masked)
    st = NumpyWeightedChi2(d["y"], d["v"])
    curves = np.random.RandomState(nx).uniform(-0.1, 0.3, size=(B, nx))
    want = st.loglike_batch_long(curves)
    assert rel_bound(nx) < 1e-12 and rel_bound(4096) < 1e-12
    for b in range(B):
        for k in range(ndata):
            got = chain(curves[b], st.y[:, k], st.w[:, k])
            assert abs(np.longdouble(got) - want[b, k]) <= rel_bound(nx) * abs(want[b, k]), (b, k, got, want[b, k])
    # the float64 statement (numpy's own summation order) is another rounding of the same sum
    assert np.allclose(st.loglike_batch(curves), want.astype(float), rtol=1e-12, atol=0)


def test_masking_rule():
    y = np.array([[1.0, np.nan, 3.0], [np.inf, 5.0, 6.0], [7.0, 8.0, -np.inf]])
    v = np.array([[0.5, 1.0, np.inf], [1.0, np.nan, 2.0], [4.0, 1e-300, 1.0]])
    y0, v0 = y.copy(), v.copy()
    yy, vv, masked = mask_pixels(y, v)
    assert np.array_equal(y, y0, equal_nan=True) and np.array_equal(v, v0, equal_nan=True)        # copies: the caller's arrays stay
    assert np.array_equal(masked, [[False, True, True], [True, True, False], [False, False, True]])
    assert np.array_equal(yy, [[1.0, 0.0, 0.0], [0.0, 0.0, 6.0], [7.0, 8.0, 0.0]])
    assert np.array_equal(vv, [[0.5, np.inf, np.inf], [np.inf, np.inf, 2.0], [4.0, 1e-300, np.inf]])
    assert np.isfinite(yy).all() and np.array_equal(1.0 / vv == 0, masked)
    for bad in (0.0, -1.0, -np.inf):
        v1 = v0.copy()
        v1[2, 0] = bad
        with pytest.raises(ValueError) as e:
            mask_pixels(y0, v1)
        assert "[2, 0]" in str(e.value)
    with pytest.raises(ValueError):
        mask_pixels(y0, v0[:2])
    # a bad value under a pixel that is masked anyway (y not finite) is not looked at
    v1 = v0.copy()
    v1[0, 1] = -1.0
    assert mask_pixels(y0, v1)[2][0, 1]
    st = NumpyWeightedChi2(y0, v0)
    assert np.array_equal(st.n_masked, [1, 2, 2])
    # a masked pixel contributes nothing, whatever the curve says there
    a = st.loglike_batch(np.array([[1.5, 2.5, 3.5]]))
    b = st.loglike_batch(np.array([[1.5, -1e6, 3.5]]))
    assert a[0, 0] == b[0, 0] and a[0, 0] == -0.5 * ((1.5 - 1.0) ** 2 / 0.5 + (3.5 - 7.0) ** 2 / 4.0)


def _case(ndata=12):
    d = weighted_data(ndata, 160, seed=3, masked=True)
    return d["x"][96:160], np.ascontiguousarray(d["y"][96:160]), np.ascontiguousarray(d["v"][96:160])


def test_problem_over_the_statement(oracle, monkeypatch):
    """``marginalise_scale=False`` over a numpy backend: the surface of the problem, and a short analysis through the
    numpy joint state that comes out the same twice."""
    patch_neighbors(monkeypatch, oracle)
    x, y, v = _case()
    scorer = NumpyWeightedChi2(y, v)
    p = problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v, marginalise_scale=False, backend=scorer)
    assert p.marginalise_scale is False and p.ndata == 12 and p.continuum == 0
    xs = gauss_prior(np.random.RandomState(2).uniform(size=(4, 3)))
    mask = np.arange(12) % 3 != 1
    want = scorer.loglike_batch(line_model(x)(xs), mask)
    assert np.array_equal(p.multi_loglikelihood_batch(xs, mask), want)
    assert np.array_equal(p.multi_loglikelihood(xs[1], mask), want[1])
    runs = []
    for _ in range(2):
        p = problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v, marginalise_scale=False, backend=NumpyWeightedChi2(y, v))
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
    x, y, v = _case(4)
    with pytest.raises(ValueError) as e:
        problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, marginalise_scale=False, backend=NumpyWeightedChi2(y, v))
    assert "marginalise_scale" in str(e.value) and "v" in str(e.value)
    with pytest.raises(ValueError) as e:
        problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v, marginalise_scale=False, continuum=2, backend=NumpyWeightedChi2(y, v))
    assert "marginalise_scale" in str(e.value) and "continuum" in str(e.value)


def test_default_backend_gets_the_keyword_only_when_false(monkeypatch):
    x, y, v = _case(4)
    made = []

    def as_before(x, y, noise_level, v=None):                     # the signature callers wrote before the switch existed
        made.append(("before", v is not None))
        return NumpyScaleMarginalised(y, v)

    def with_keywords(x, y, noise_level, v=None, **kw):
        made.append(("keywords", v is not None, dict(kw)))
        return NumpyWeightedChi2(y, v)
    monkeypatch.setattr(problem, "default_backend", as_before)
    p = problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v)
    assert p.marginalise_scale is True and isinstance(p.backend, NumpyScaleMarginalised)
    problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v, marginalise_scale=True)
    with pytest.raises(TypeError):                                # the old signature cannot take the new keyword: it is sent
        problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v, marginalise_scale=False)
    monkeypatch.setattr(problem, "default_backend", with_keywords)
    problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v)
    p = problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, v=v, marginalise_scale=False)
    assert isinstance(p.backend, NumpyWeightedChi2)
    assert made == [("before", True), ("before", True), ("keywords", True, {}), ("keywords", True, {"marginalise_scale": False})]


MODEL_FILE = """
import numpy
x = numpy.linspace(400, 800, 200)[96:160]
ndim = 3
marginalise_scale = False
def priortransform_batch(us):
    us = numpy.asarray(us, dtype=float)
    return numpy.column_stack((10 ** (us[:, 0] * 2 - 2), us[:, 1] * 400 + 400, 10 ** (us[:, 2] * 2)))
def model(xs):
    return numpy.array([A * numpy.exp(-0.5 * ((mu - x) / sig) ** 2) for A, mu, sig in xs]).reshape(len(xs), len(x))
"""


def _write_case(tmp_path, with_v):
    x, y, v = _case(6)
    data = str(tmp_path / "data.npz")
    gen.save(data, dict(x=x, y=y, v=v) if with_v else dict(x=x, y=y))
    path = tmp_path / "mymodel.py"
    path.write_text(MODEL_FILE)
    return data, str(path)


def test_load_model_returns_the_switch(tmp_path):
    _, path = _write_case(tmp_path, True)
    assert sample.load_model(path)["marginalise_scale"] is False
    other = tmp_path / "other.py"
    other.write_text(MODEL_FILE.replace("marginalise_scale = False\n", ""))
    assert sample.load_model(str(other))["marginalise_scale"] is True


def test_mdns_model_drives_main_at_fixed_scale(tmp_path, oracle, monkeypatch, capsys):
    patch_neighbors(monkeypatch, oracle)
    data, path = _write_case(tmp_path, True)
    made = []

    def backend(x, y, noise_level, v=None, **kw):
        made.append((len(x), y.shape, v.shape, dict(kw)))
        return NumpyWeightedChi2(y, v)
    monkeypatch.setattr(problem, "default_backend", backend)
    monkeypatch.setenv("MDNS_MODEL", path)
    monkeypatch.setenv("NLIVE_POINTS", "20")
    monkeypatch.setenv("MAXSAMPLES", "30")
    monkeypatch.setenv("USE_GRAPH", "0")
    monkeypatch.delenv("MDNS_POSTERIOR", raising=False)
    sample.main(["sample", data, "6"])
    assert made == [(64, (64, 6), (64, 6), {"marginalise_scale": False})]
    out = capsys.readouterr().out
    assert "logZ = " in out and "ndraws:" in out
    written = gen.read_datasets(data + "_MLFRIENDS_nlive20_6.out8.npz")
    assert written["logZ"].shape == (6,) and np.isfinite(written["logZ"]).all() and int(written["ndraws"]) > 0


def test_mdns_model_at_fixed_scale_needs_variances(tmp_path, monkeypatch):
    data, path = _write_case(tmp_path, False)
    monkeypatch.setenv("MDNS_MODEL", path)
    with pytest.raises(SystemExit) as e:
        sample.main(["sample", data, "6"])
    assert e.value.code not in (0, None) and "marginalise_scale" in str(e.value.code) and "`v`" in str(e.value.code)


def test_the_amplitude_is_measured_only_at_fixed_scale():
    """What the likelihood is for.  12 spectra hold the same line at 12 amplitudes; over a grid of 41 amplitudes around
    each truth (mu and sig at their true values) the fixed-scale statement peaks at the grid point nearest the truth,
    for all 12, while the scale-marginalised one does not see the amplitude at all.

    The chosen signal-to-noise: sigma = 0.01 (1 + 3 u) per pixel, a line of width 8 nm (4 channels) with amplitudes
    5.0, 5.25 ... 7.75, grid spacing 0.2 (every grid amplitude is positive).  The maximum-likelihood amplitude scatters by sigma_A = (sum_j w_j g_j^2)^-1/2
    around the truth, which is a grid point: the peak is off by one when |A^ - A| > 0.1.  sigma_A <= 0.0125 for every
    spectrum here (asserted below from the weights alone), so that is an 8 sigma event."""
    ndata, nx = 12, 64
    x = gen.horns(1)["x"][96:96 + nx]
    mu, sig = float(x[nx // 2]) + 0.7, 8.0
    rng = np.random.RandomState(12)
    sigma = 0.01 * (1 + 3 * rng.uniform(size=(nx, ndata)))
    g = np.exp(-0.5 * ((mu - x) / sig) ** 2)
    truth = 5.0 + 0.25 * np.arange(ndata)
    y = truth[None, :] * g[:, None] + sigma * rng.normal(size=(nx, ndata))
    v = sigma ** 2
    sigma_A = ((g[:, None] ** 2 / v).sum(axis=0)) ** -0.5
    step = 0.2
    assert sigma_A.max() <= 0.0125 and step / 2 >= 8 * sigma_A.max()
    fixed, marginal = NumpyWeightedChi2(y, v), NumpyScaleMarginalised(y, v)
    for k in range(ndata):
        grid = truth[k] + step * (np.arange(41) - 20)
        sel = np.arange(ndata) == k
        curves = grid[:, None] * g[None, :]
        L = fixed.loglike_batch(curves, sel)[:, 0]
        assert int(np.argmax(L)) == 20, (k, int(np.argmax(L)))
        assert L[20] - max(L[19], L[21]) > 1.0                              # a peak, not a tie
        Lm = marginal.loglike_batch(curves, sel)[:, 0]
        assert np.max(np.abs(Lm - Lm[0])) <= 1e-6 * np.abs(Lm[0]), k
