"""The table model on the CPU tier (massivedatans_amd/tablemodel.py): ``TableModel.statement`` against the independent
form ``A * numpy.interp(x / (1 + z), grid, multilinear template)`` within the bound table_support derives, the edges of
the statement, ``problem.CurveProblem`` with a TableModel over a numpy scorer against the same run given the statement
as a plain model, parameter recovery, and every refusal of TableModel, CurveProblem and ``sample.load_model``."""
import numpy as np
import pytest

from massivedatans_amd import jointstate, problem, sample
from massivedatans_amd.tablemodel import TableModel
from curves_support import NumpyFixedNoise
from oracle_backend import patch_neighbors
from table_support import abscissa, bound, edge_params, independent, make_model, posterior_moments, random_params, same_bits


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_statement_against_the_independent_form(d):
    """Uneven axes and grid, parameters inside and outside the axes, z in [0, 0.5], amplitudes over two decades, channels
    past both ends of the grid; all four flag combinations.  The worst error as a share of the bound is printed."""
    worst = 0.0
    for redshift in (False, True):
        for amplitude in (False, True):
            tm = make_model(d, seed=10 * d + 2 * redshift + amplitude, nw=60, redshift=redshift, amplitude=amplitude)
            assert tm.ndim == d + redshift + amplitude
            x = abscissa(tm, 200, seed=d)
            xs = random_params(tm, np.random.RandomState(d), 64)
            got, want = tm.statement(x, xs), independent(tm, x, xs)
            assert got.shape == (64, 200) and np.isfinite(got).all()
            ratio = float((np.abs(got - want) / bound(tm, xs)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (d, redshift, amplitude, ratio)
    print("d=%d: worst |statement - independent| = %.3g of the bound" % (d, worst))
    assert worst > 0                      # (two orders of the same polynomial do differ in the last bits somewhere)


def test_the_issues_shape_agrees_to_a_few_eps():
    """A 5 x 7 x 3 x 2000 table, 200 channels, z in [0, 0.5], amplitudes over two decades: relative to the largest value
    of a curve the two forms agree to a few 1e-16."""
    tm = make_model(3, seed=3, lengths=[5, 7, 3], nw=2000)
    x = abscissa(tm, 200, seed=1, beyond=0.0)
    xs = random_params(tm, np.random.RandomState(4), 32, beyond=0.0)
    got, want = tm.statement(x, xs), independent(tm, x, xs)
    rel = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    print("relative difference %.3g" % rel)
    assert rel < 5e-15 and (np.abs(got - want) <= bound(tm, xs)).all()


def test_the_edges_of_the_statement():
    tm = make_model(2, seed=5, lengths=[2, 4], nw=9)
    x = abscissa(tm, 33, seed=2)
    xs, names, first_nan = edge_params(tm, x)
    with np.errstate(all="ignore"):
        got = tm.statement(x, xs)
    # a NaN anywhere in a candidate: its whole row, and no other row
    assert np.isnan(got[first_nan:]).all() and len(got) - first_nan == tm.ndim
    rows = dict(zip(names, got))
    mid = [0.5 * (a[0] + a[1]) for a in tm.axes]
    at = lambda p0, p1, z=0.25, A=1.5: tm.statement(x, np.array([[p0, p1, z, A]]))[0]
    # outside an axis is its end; +-inf clamps
    for a, axis in enumerate(tm.axes):
        for name, v in (("below", axis[0]), ("-inf", axis[0]), ("above", axis[-1]), ("+inf", axis[-1])):
            p = list(mid)
            p[a] = v
            assert same_bits(rows["axis %d %s" % (a, name)], at(*p)), (a, name)
    # on knots the table's own rows come back exactly (weights 1 and 0, t = 0) -- but for the last grid knot, which is
    # read from the cell before it at t = 1: T0 + 1 (T1 - T0), one rounding away from T1
    on_knots = tm.statement(tm.grid, np.array([[tm.axes[0][0], tm.axes[1][0], 0.0, 1.0], [tm.axes[0][-1], tm.axes[1][-1], 0.0, 1.0]]))
    assert np.array_equal(on_knots[0][:-1], tm.table[0, 0][:-1]) and np.array_equal(on_knots[1][:-1], tm.table[-1, -1][:-1])
    assert np.allclose(on_knots[:, -1], [tm.table[0, 0, -1], tm.table[-1, -1, -1]], rtol=1e-15, atol=1e-15)
    # numpy.interp's end rules along the grid; z = -1 divides by zero and clamps
    assert (rows["every u below the grid"] == rows["every u below the grid"][0]).all()
    assert (rows["every u above the grid"] == rows["every u above the grid"][0]).all()
    assert same_bits(rows["z = -1"], rows["every u above the grid"]) and same_bits(rows["z = +inf"], rows["every u below the grid"])
    assert same_bits(rows["A = 0"], 0.0 * at(*mid, A=1.0))
    assert same_bits(rows["A = -2"], -2.0 * at(*mid, A=1.0))
    # a candidate's curve does not depend on its batch
    assert same_bits(tm.statement(x, xs[3:4])[0], got[3]) and same_bits(tm.statement(x, xs[::-1])[::-1], got)


def _prior(tm, zmax=0.1):
    lo = np.array([a[0] for a in tm.axes] + ([0.0] if tm.redshift else []) + ([-1.0] if tm.amplitude else []))
    hi = np.array([a[-1] for a in tm.axes] + ([zmax] if tm.redshift else []) + ([1.0] if tm.amplitude else []))

    def priortransform_batch(us):
        xs = lo + (hi - lo) * np.asarray(us, dtype=float)
        if tm.amplitude:
            xs[:, -1] = 10 ** xs[:, -1]
        return xs
    return priortransform_batch


def _data(tm, x, truth, noise, seed):
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray((tm.statement(x, truth) + noise * rng.normal(size=(len(truth), len(x)))).T)


def _run(p, nlive, max_samples):
    sampler = sample.build_sampler(p, nlive_points=nlive, nsuperset_draws=10, use_graph=False, seed=1, fused=True)
    with np.errstate(all="ignore"):
        results = sample.integrate(sampler, 0.5, 0, max_samples)
    return results, sampler


def test_problem_with_a_table_model_equals_its_statement_as_a_plain_model(oracle, monkeypatch):
    patch_neighbors(monkeypatch, oracle)
    tm = make_model(2, seed=7, lengths=[3, 4], nw=30)
    x = abscissa(tm, 40, seed=3, beyond=0.0)
    prior = _prior(tm)
    truth = prior(np.random.RandomState(1).uniform(0.2, 0.8, size=(6, tm.ndim)))
    y = _data(tm, x, truth, 0.05, seed=2)
    runs = []
    for model in (tm, lambda xs: tm.statement(x, xs)):
        p = problem.CurveProblem(x, y, model, prior, tm.ndim, noise_level=0.05, backend=NumpyFixedNoise(y, 0.05))
        assert p.table is None
        results, sampler = _run(p, 20, 40)
        assert isinstance(sampler.joint, jointstate.HostJointState) and sampler.ndraws > 0
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert np.isfinite(runs[0][0]).all() and runs[0][2] == runs[1][2]
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    # the non-draw path is the statement too
    p = problem.CurveProblem(x, y, tm, prior, tm.ndim, noise_level=0.05, backend=NumpyFixedNoise(y, 0.05))
    mask = np.array([True, False, True, True, False, True])
    assert np.array_equal(p.multi_loglikelihood_batch(truth, mask), NumpyFixedNoise(y, 0.05).loglike_batch(tm.statement(x, truth), mask))


RECOVERY_FACTOR = 4.0


def test_parameter_recovery(oracle, monkeypatch):
    """Spectra made from the table at known (p, z, A) plus noise at the stated level: the posterior mean of every
    parameter of every data set lies within RECOVERY_FACTOR posterior standard deviations of the truth.  (A Gaussian
    posterior puts the truth beyond 4 of its standard deviations from the mean once in 16 000 cases; 4 data sets x 3
    parameters are 12.)  The table is monotone along its axis, so the parameter is identified."""
    patch_neighbors(monkeypatch, oracle)
    rng = np.random.RandomState(3)
    axis = np.array([0.0, 0.4, 1.0, 1.5, 2.5])
    grid = np.sort(np.concatenate(([300.0, 900.0], rng.uniform(300, 900, size=48))))
    table = 1.0 + np.exp(-0.5 * ((grid[None, :] - 600.0) / (20.0 + 30.0 * axis[:, None])) ** 2) * (1.0 + axis[:, None])
    tm = TableModel([axis], grid, table, redshift=True, amplitude=True)
    x = np.linspace(420.0, 860.0, 48)
    prior = _prior(tm, zmax=0.1)
    truth = np.array([[0.7, 0.03, 1.2], [1.8, 0.06, 0.5], [0.3, 0.08, 3.0], [2.2, 0.02, 2.0]])
    noise = 0.05
    y = _data(tm, x, truth, noise, seed=5)
    p = problem.CurveProblem(x, y, tm, prior, tm.ndim, noise_level=noise, backend=NumpyFixedNoise(y, noise))
    results, sampler = _run(p, 100, 0)
    mean, std = posterior_moments(results)
    pull = np.abs(mean - truth) / std
    print("posterior mean - truth in posterior standard deviations:\n%s" % np.round(pull, 2))
    assert np.isfinite(results["logZ"]).all() and (std > 0).all()
    assert (pull < RECOVERY_FACTOR).all(), pull


def test_table_model_refusals():
    axis, grid = np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0, 3.0, 5.0])
    table = np.ones((3, 4))
    assert TableModel([axis], grid, table).ndim == 1 and TableModel([axis], grid, table, True, True).ndim == 3
    bad = [
        dict(axes=[], grid=grid, table=table),                                       # d = 0
        dict(axes=[axis] * 5, grid=grid, table=np.ones((3, 3, 3, 3, 3, 4))),            # d = 5
        dict(axes=[axis[:1]], grid=grid, table=np.ones((1, 4))),                     # an axis of one knot
        dict(axes=[axis[::-1]], grid=grid, table=table),                             # decreasing
        dict(axes=[np.array([0.0, 1.0, 1.0])], grid=grid, table=table),              # not strictly increasing
        dict(axes=[np.array([0.0, 1.0, np.inf])], grid=grid, table=table),           # not finite
        dict(axes=[np.array([0.0, np.nan, 2.0])], grid=grid, table=table),
        dict(axes=[axis.reshape(3, 1)], grid=grid, table=table),                     # not one-dimensional
        dict(axes=[axis], grid=grid[:1], table=np.ones((3, 1))),                     # nw = 1
        dict(axes=[axis], grid=np.array([1.0, 3.0, 2.0, 5.0]), table=table),
        dict(axes=[axis], grid=np.array([1.0, 2.0, 3.0, np.inf]), table=table),
        dict(axes=[axis], grid=grid, table=np.ones((4, 3))),                         # shape
        dict(axes=[axis], grid=grid, table=np.ones((3, 4, 1))),
        dict(axes=[axis], grid=grid, table=np.where(np.eye(3, 4) > 0, np.nan, 1.0)),
        dict(axes=[axis], grid=grid, table=np.where(np.eye(3, 4) > 0, -np.inf, 1.0)),
        dict(axes=3.0, grid=grid, table=table),                                      # not a sequence
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            TableModel(**kw)
    tm = TableModel([axis], grid, table, redshift=True)
    for xs in (np.ones((2, 1)), np.ones((2, 3)), np.ones((2, 2, 2))):
        with pytest.raises(ValueError):
            tm.statement(grid, xs)
    with pytest.raises(ValueError):
        tm.statement(np.ones((2, 2)), np.ones((1, 2)))


def test_problem_and_model_file_refusals(tmp_path):
    tm = make_model(2, seed=1, lengths=[2, 3], nw=5)
    x = abscissa(tm, 8)
    y = np.zeros((8, 3))
    scorer = NumpyFixedNoise(y, 1.0)
    for ndim in (tm.ndim - 1, tm.ndim + 1, 2):
        with pytest.raises(ValueError) as e:
            problem.CurveProblem(x, y, tm, _prior(tm), ndim, backend=scorer)
        assert "table model" in str(e.value)
    assert problem.CurveProblem(x, y, tm, _prior(tm), tm.ndim, backend=scorer).nparams == tm.ndim
    text = """
import numpy
from massivedatans_amd.tablemodel import TableModel
model = TableModel([numpy.array([0.0, 1.0])], numpy.array([1.0, 2.0, 3.0]), numpy.ones((2, 3)), redshift=True)
ndim = %s
def priortransform_batch(us):
    return numpy.asarray(us, dtype=float)
"""
    good = tmp_path / "table_ok.py"
    good.write_text(text % "2")
    got = sample.load_model(str(good))
    assert isinstance(got["model"], TableModel) and got["ndim"] == 2
    for value in ("3", "1", "'two'"):
        wrong = tmp_path / "table_wrong.py"
        wrong.write_text(text % value)
        with pytest.raises(ValueError) as e:
            sample.load_model(str(wrong))
        assert "ndim" in str(e.value) and "table_wrong.py" in str(e.value)


def test_a_wrong_ndim_in_a_model_file_ends_the_program(tmp_path, monkeypatch):
    path = tmp_path / "table_wrong.py"
    path.write_text("import numpy\nfrom massivedatans_amd.tablemodel import TableModel\n"
                    "model = TableModel([numpy.array([0.0, 1.0])], numpy.array([1.0, 2.0]), numpy.ones((2, 2)))\nndim = 4\n"
                    "def priortransform_batch(us):\n    return us\n")
    monkeypatch.setenv("MDNS_MODEL", str(path))
    with pytest.raises(SystemExit) as e:
        sample.main(["sample", "nowhere.npz", "3"])
    assert e.value.code not in (0, None) and "MDNS_MODEL" in str(e.value.code) and "table model takes 1" in str(e.value.code)
