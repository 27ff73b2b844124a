"""Caller-defined models on the CPU tier: ``problem.CurveProblem`` over a numpy scorer -- the joint state
is then ``jointstate.HostJointState`` -- through ``sample.build_sampler(fused=True)``, on the native
constrainer and the native core where libmdns_host.so is built; and the ``MDNS_MODEL`` switch of
``python -m massivedatans_amd.sample``."""
import numpy as np
import pytest

from massivedatans_amd import constrainer, gen, jointstate, problem, sample
from curves_support import NumpyFixedNoise, NumpyScaleMarginalised, gauss_prior, line_model, muse_cut, muse_line_model, muse_prior
from oracle_backend import patch_neighbors


def _analyse(p, nlive=20, max_samples=40):
    sampler = sample.build_sampler(p, nlive_points=nlive, nsuperset_draws=10, use_graph=False, seed=1, fused=True)
    with np.errstate(all="ignore"):
        results = sample.integrate(sampler, 0.5, 0, max_samples)
    accepted = np.array(sampler.pointpilex[:int(len(sampler.pointpilex))])
    return results, sampler, accepted


def _check_run(make_problem):
    runs = []
    for _ in range(2):
        p = make_problem()
        results, sampler, accepted = _analyse(p)
        assert isinstance(sampler.joint, jointstate.HostJointState)
        if constrainer.available():
            assert sampler.native is not None and type(sampler).__name__ == "NativeCoreSampler"
        assert results["logZ"].shape == (p.ndata,) and np.isfinite(results["logZ"]).all()
        assert sampler.ndraws > 0
        runs.append((results["logZ"], int(sampler.ndraws), accepted))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    assert np.array_equal(runs[0][2], runs[1][2])


def test_complete_small_analysis(oracle, monkeypatch):
    patch_neighbors(monkeypatch, oracle)
    d = gen.horns(12)
    x, y = d["x"][96:160], np.ascontiguousarray(d["y"][96:160])          # 64 channels around the lines
    _check_run(lambda: problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, noise_level=0.01,
                                            backend=NumpyFixedNoise(y, 0.01)))


def test_scale_marginalised_form(oracle, monkeypatch):
    """``v`` given and noise on every evaluation, as musefuse.py:520-535."""
    patch_neighbors(monkeypatch, oracle)
    d = muse_cut(8, 96)
    _check_run(lambda: problem.CurveProblem(d["x"], d["y"], muse_line_model(d["x"]), muse_prior, 3, v=d["v"], jitter_sigma=1e-5,
                                            backend=NumpyScaleMarginalised(d["y"], d["v"])))


def test_problem_surface():
    d = gen.horns(5)
    x, y = d["x"][:64], np.ascontiguousarray(d["y"][:64])
    scorer = NumpyFixedNoise(y, 0.01)
    p = problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, backend=scorer)
    assert p.ndata == 5 and p.nparams == 3
    u = np.array([0.3, 0.6, 0.2])
    assert np.array_equal(p.priortransform(u), gauss_prior(u[None])[0])
    xs = gauss_prior(np.random.RandomState(2).uniform(size=(4, 3)))
    mask = np.array([True, False, True, True, False])
    want = scorer.loglike_batch(line_model(x)(xs), mask)
    assert np.array_equal(p.multi_loglikelihood_batch(xs, mask), want)
    assert np.array_equal(p.multi_loglikelihood(xs[1], mask), want[1])
    prior = p.native_prior()
    assert prior.ndim == 3 and prior.nparams == 3 and prior.jitter_sigma == 0 and bool(prior.custom)
    assert problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, backend=scorer, jitter_sigma=1e-5).multi_loglikelihood_batch is None
    with pytest.raises(ValueError):
        problem.CurveProblem(x, y, line_model(x), gauss_prior, 17, backend=scorer)


MODEL_FILE = """
import numpy
x = numpy.linspace(400, 800, 200)[96:160]
ndim = 3
noise_level = 0.01
def priortransform_batch(us):
    us = numpy.asarray(us, dtype=float)
    return numpy.column_stack((10 ** (us[:, 0] * 2 - 2), us[:, 1] * 400 + 400, 10 ** (us[:, 2] * 2)))
def model(xs):
    return numpy.array([A * numpy.exp(-0.5 * ((mu - x) / sig) ** 2) for A, mu, sig in xs]).reshape(len(xs), len(x))
"""


def _write_case(tmp_path, text):
    d = gen.horns(6)
    data = str(tmp_path / "data.npz")
    gen.save(data, dict(x=d["x"][96:160], y=np.ascontiguousarray(d["y"][96:160])))
    path = tmp_path / "mymodel.py"
    path.write_text(text)
    return data, str(path)


def test_mdns_model_drives_main(tmp_path, oracle, monkeypatch, capsys):
    patch_neighbors(monkeypatch, oracle)
    data, path = _write_case(tmp_path, MODEL_FILE)
    made = []

    def backend(x, y, noise_level, v=None):
        made.append((len(x), y.shape, noise_level, v))
        return NumpyFixedNoise(y, noise_level)
    monkeypatch.setattr(problem, "default_backend", backend)
    monkeypatch.setenv("MDNS_MODEL", path)
    monkeypatch.setenv("NLIVE_POINTS", "20")
    monkeypatch.setenv("MAXSAMPLES", "30")
    monkeypatch.setenv("USE_GRAPH", "0")
    monkeypatch.delenv("MDNS_POSTERIOR", raising=False)
    sample.main(["sample", data, "6"])
    assert made == [(64, (64, 6), 0.01, None)]
    out = capsys.readouterr().out
    assert "logZ = " in out and "ndraws:" in out
    written = gen.read_datasets(data + "_MLFRIENDS_nlive20_6.out8.npz")
    assert written["logZ"].shape == (6,) and np.isfinite(written["logZ"]).all() and int(written["ndraws"]) > 0


def test_mdns_model_file_without_a_model(tmp_path, monkeypatch):
    data, path = _write_case(tmp_path, MODEL_FILE.replace("def model(", "def shape("))
    monkeypatch.setenv("MDNS_MODEL", path)
    with pytest.raises(SystemExit) as e:
        sample.main(["sample", data, "6"])
    assert e.value.code not in (0, None) and "`model`" in str(e.value.code) and "mymodel.py" in str(e.value.code)
