"""The sum model's numpy statement (massivedatans_amd/summodel.py, include/mdns.h Part 14) on the CPU: against the
independent formulae within a derived bound, its exact facts, the NaN rules, ``SumModel``'s refusals, a whole run over a
numpy scorer against the same statement as a plain function, and model files."""
import numpy as np
import pytest

from massivedatans_amd import _host, jointstate, problem, sample
from massivedatans_amd.summodel import GaussianLine, PowerLaw, SumModel
from curves_support import NumpyFixedNoise
from oracle_backend import patch_neighbors
from sum_support import EPS, attenuation, edge_rows, independent, los_table, model_params, positive_prior, positive_sum, rule_rows, table
from table_support import abscissa, same_bits

X = np.linspace(310.0, 890.0, 41)


def _models():
    t1, t2 = table(1, 3), table(2, 4, redshift=False)
    bare = [table(1, 11 + k, redshift=False, amplitude=False) for k in range(2)]        # one parameter each: 8 components in 15
    return [
        ("power law", SumModel([PowerLaw(x0=500.0)])),
        ("line", SumModel([GaussianLine()])),
        ("table", SumModel([t1])),
        ("all three, attenuated", SumModel([PowerLaw(x0=600.0), GaussianLine(), t1], attenuation=attenuation(X))),
        ("mixed", SumModel([t2, GaussianLine(), PowerLaw(), GaussianLine()], attenuation=attenuation(X, 1), unattenuated=[0, 3])),
        ("none attenuated", SumModel([GaussianLine(), PowerLaw(x0=400.0)], attenuation=attenuation(X, 2), unattenuated=[0, 1])),
        ("eight", SumModel([PowerLaw(x0=450.0), GaussianLine(), bare[0], bare[1]] * 2, attenuation=attenuation(X, 3), unattenuated=[1, 4, 6])),
    ]


@pytest.mark.parametrize("name,sm", _models(), ids=[m[0] for m in _models()])
def test_statement_against_the_independent_forms(name, sm):
    """|statement - independent| within the bound derived in sum_support, wherever every exponent has |q| <= 200."""
    xs = model_params(sm, X, np.random.RandomState(len(name)), 40)
    got = sm.statement(X, xs)
    want, bound, ok = independent(sm, X, xs)
    assert got.shape == want.shape == (40, len(X)) and ok.mean() > 0.5 and np.isfinite(got).all()
    worst = np.max(np.abs(got - want)[ok] / bound[ok])
    rel = np.max(np.abs(got - want)[ok] / np.maximum(np.abs(want[ok]), 1e-300))
    print("%s: worst |diff| / bound = %.3f, largest relative difference %.2e, %d of %d bins compared" % (name, worst, rel, ok.sum(), ok.size))
    assert worst <= 1.0


def test_exact_facts_of_the_analytic_components():
    x = np.array([1.0, 2.0, 10.0, 17.5, 40.0])
    line = SumModel([GaussianLine()])
    got = line.statement(x, [[3.7, 17.5, 2.0], [-0.3, 10.0, 1e-320], [2.5, 3.0, 1e-320]])
    assert got[0, 3] == 3.7 and got[1, 2] == -0.3                       # x_j == mu: A exactly
    tiny = _host.pow10_dd(np.array([-299.0]))[0]
    assert tiny == 1e-299
    # sigma subnormal: d = +-inf, q = -299, no NaN; far from the line A * 1e-299, not 0
    assert not np.isnan(got).any() and same_bits(got[2], np.full(5, 2.5 * tiny)) and same_bits(got[1, [0, 1, 3, 4]], np.full(4, -0.3 * tiny))
    # lx_j = 1, logA = 0: G = 299 on the clamp, G = 300 beyond it
    pl = SumModel([PowerLaw(x0=1.0)])
    assert pl.components[0].lx(x)[2] == 1.0
    on, beyond = pl.statement(x, [[0.0, 299.0], [0.0, 300.0]])[:, 2]
    assert on == beyond == 1e-299
    assert pl.statement(x, [[0.0, 0.0]])[0, 0] == 1.0 and pl.statement(x, [[-0.0, -0.0]])[0, 4] == 1.0   # pow10_dd(+-0.0) = 1


def test_n_zero_gives_the_unattenuated_sum():
    comps = [PowerLaw(x0=500.0), GaussianLine(), table(2, 5)]
    plain, with_att = SumModel(comps), SumModel(comps, attenuation=attenuation(X))
    xs = model_params(plain, X, np.random.RandomState(1), 9)
    want = plain.statement(X, xs)
    for N in (0.0, -0.0):
        assert same_bits(with_att.statement(X, np.column_stack((xs, np.full(9, N)))), want)


def test_a_lone_table_is_the_tables_statement():
    for tm in (table(3, 7), los_table(2, 8, nw=30)):
        sm = SumModel([tm])
        x = abscissa(tm, 37, seed=1)
        xs = model_params(sm, x, np.random.RandomState(2), 12)
        xs[3, -1], xs[4, -1] = -0.0, 0.0                                   # A = -0.0: the table's curve holds -0.0 (or +0.0)
        with np.errstate(all="ignore"):
            own = tm.statement(x, xs)
            got = sm.statement(x, xs)
        assert np.signbit(own[3:5]).any() and not np.signbit(got[3:5]).any()
        assert same_bits(got, own + 0.0) and sm.ndim == tm.ndim and sm.slices == [slice(0, tm.ndim)]


def test_permuting_components_changes_only_the_order_of_the_adds():
    rng = np.random.RandomState(4)
    a, b, c = GaussianLine(), PowerLaw(x0=500.0), table(1, 9)
    two, owt = SumModel([a, b]), SumModel([b, a])
    xs = model_params(two, X, rng, 20)
    assert same_bits(two.statement(X, xs), owt.statement(X, xs[:, [3, 4, 0, 1, 2]]))       # 0 + v1 + v2 is commutative
    three = SumModel([a, b, c])
    xs = model_params(three, X, rng, 20)
    parts = [xs[:, sl] for sl in three.slices]
    values = [np.abs(SumModel([k]).statement(X, p)) for k, p in zip((a, b, c), parts)]
    for order in ((2, 0, 1), (1, 2, 0), (2, 1, 0)):
        other = SumModel([(a, b, c)[k] for k in order])
        diff = np.abs(other.statement(X, np.column_stack([parts[k] for k in order])) - three.statement(X, xs))
        assert (diff <= 2 * 3 * EPS * sum(values)).all(), order


def test_the_nan_rules_parameter_by_parameter():
    for name, sm in _models():
        rng = np.random.RandomState(7)
        good = model_params(sm, X, rng, 6, positive=True)
        bad, names = rule_rows(sm, X, good[0])
        edges, edge_names = edge_rows(sm, X, good[1])
        batch = np.vstack((good[:3], bad, good[3:], edges))
        with np.errstate(all="ignore"):
            got = sm.statement(X, batch)
            alone = sm.statement(X, good)
            edge_alone = np.vstack([sm.statement(X, e[None]) for e in edges]) if len(edges) else np.empty((0, len(X)))
        nb = len(bad)
        for k, what in enumerate(names):
            assert np.isnan(got[3 + k]).all(), (name, what)
        assert same_bits(got[:3], alone[:3]) and same_bits(got[3 + nb:6 + nb], alone[3:]) and np.isfinite(alone).all(), name
        # rows on the edges: no NaN from finite parameters, and the same bits alone as in the batch
        assert same_bits(got[6 + nb:], edge_alone), name
        for k, what in enumerate(edge_names):
            assert not np.isnan(edge_alone[k]).any(), (name, what)


def test_sum_model_refusals():
    g, pl, tm = GaussianLine(), PowerLaw(), table(1, 1)
    for comps, words in (([], "0 components"), ([g] * 9, "9 components"), ([g] * 6, "18 parameters"), ([g, "line"], "component 1"),
                         (g, "sequence")):
        with pytest.raises(ValueError) as e:
            SumModel(comps)
        assert words in str(e.value), str(e.value)
    assert SumModel([g] * 5, attenuation=np.zeros(4)).ndim == 16
    with pytest.raises(ValueError) as e:
        SumModel([g] * 4 + [pl, pl], attenuation=np.zeros(4))              # 12 + 4 + 1
    assert "17 parameters" in str(e.value)
    for bad in ([2], [-1], [0.5]):
        with pytest.raises(ValueError) as e:
            SumModel([g, pl], attenuation=np.zeros(4), unattenuated=bad)
        assert "unattenuated" in str(e.value)
    with pytest.raises(ValueError) as e:
        SumModel([g], attenuation=[0.0, np.inf])
    assert "attenuation[1]" in str(e.value)
    with pytest.raises(ValueError):
        PowerLaw(x0=0.0)
    sm = SumModel([g, pl, tm], attenuation=np.zeros(5), unattenuated=[1])
    assert sm.ndim == 3 + 2 + tm.ndim + 1 and sm.slices == [slice(0, 3), slice(3, 5), slice(5, 5 + tm.ndim)] and sm.attenuated == [True, False, True]
    x5 = np.linspace(1.0, 2.0, 5)
    for method in (lambda x: sm.statement(x, np.ones((1, sm.ndim))), sm.bind):
        with pytest.raises(ValueError) as e:
            method(np.linspace(1.0, 2.0, 6))
        assert "attenuation has 5 values, x has 6" in str(e.value)
        with pytest.raises(ValueError) as e:
            method(x5 - 1.0)
        assert "x > 0" in str(e.value) and "x[0]" in str(e.value)
    with pytest.raises(ValueError) as e:
        sm.statement(x5, np.ones((2, sm.ndim - 1)))
    assert "[B, %d]" % sm.ndim in str(e.value)
    assert SumModel([g, tm]).statement(x5 - 1.0, np.ones((1, 3 + tm.ndim))).shape == (1, 5)     # without a power law any x


_prior = positive_prior


def test_problem_and_model_file(tmp_path):
    x = np.linspace(420.0, 880.0, 33)
    sm = positive_sum(x)
    y = np.zeros((33, 3))
    scorer = NumpyFixedNoise(y, 1.0)
    for ndim in (sm.ndim - 1, sm.ndim + 1):
        with pytest.raises(ValueError) as e:
            problem.CurveProblem(x, y, sm, _prior(sm), ndim, backend=scorer)
        assert "the sum model takes 10 parameters" in str(e.value)
    p = problem.CurveProblem(x, y, sm, _prior(sm), sm.ndim, backend=scorer)
    assert p.nparams == 10 and p.table is None
    text = """
import numpy
from massivedatans_amd.summodel import SumModel, PowerLaw, GaussianLine
from massivedatans_amd.tablemodel import TableModel
tm = TableModel([numpy.array([0.0, 1.0])], numpy.array([1.0, 2.0, 3.0]), numpy.ones((2, 3)), amplitude=True)
model = SumModel([PowerLaw(x0=2.0), GaussianLine(), tm], attenuation=numpy.zeros(7), unattenuated=[2])
ndim = %s
def priortransform_batch(us):
    return numpy.asarray(us, dtype=float)
"""
    good = tmp_path / "sum_ok.py"
    good.write_text(text % "8")
    got = sample.load_model(str(good))
    assert isinstance(got["model"], SumModel) and got["ndim"] == 8 and got["model"].attenuated == [True, True, False]
    for value in ("7", "9"):
        wrong = tmp_path / "sum_wrong.py"
        wrong.write_text(text % value)
        with pytest.raises(ValueError) as e:
            sample.load_model(str(wrong))
        assert "ndim" in str(e.value) and "sum model takes 8" in str(e.value)


def test_a_whole_run_equals_the_statement_as_a_plain_model(oracle, monkeypatch):
    """64 spectra, nx 33, 50 live points, 60 samples over a numpy scorer (the state is HostJointState): the SumModel and
    its statement wrapped as a plain function give the same draws, points and logZ."""
    patch_neighbors(monkeypatch, oracle)
    x = np.linspace(420.0, 880.0, 33)
    sm = positive_sum(x)
    prior = _prior(sm)
    truth = prior(np.random.RandomState(1).uniform(0.2, 0.8, size=(64, sm.ndim)))
    y = np.ascontiguousarray((sm.statement(x, truth) + 0.2 * np.random.RandomState(2).normal(size=(64, 33))).T)
    runs = []
    for model in (sm, lambda xs: sm.statement(x, xs)):
        p = problem.CurveProblem(x, y, model, prior, sm.ndim, noise_level=0.2, backend=NumpyFixedNoise(y, 0.2))
        assert p.table is None
        sampler = sample.build_sampler(p, nlive_points=50, nsuperset_draws=10, use_graph=False, seed=1, fused=True)
        with np.errstate(all="ignore"):
            results = sample.integrate(sampler, 0.5, 0, 60)
        assert isinstance(sampler.joint, jointstate.HostJointState) and sampler.ndraws > 0
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert np.isfinite(runs[0][0]).all() and runs[0][2] == runs[1][2] and runs[0][3].shape[-1] == sm.ndim
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    mask = np.arange(64) % 3 != 0
    p = problem.CurveProblem(x, y, sm, prior, sm.ndim, noise_level=0.2, backend=NumpyFixedNoise(y, 0.2))
    assert np.array_equal(p.multi_loglikelihood_batch(truth[:5], mask), NumpyFixedNoise(y, 0.2).loglike_batch(sm.statement(x, truth[:5]), mask))
