"""The table model's line-of-sight effects on the CPU tier (massivedatans_amd/tablemodel.py, csrc/host_pow10.cpp):
``_host.pow10_dd`` against the test build of the same header, ``TableModel.statement`` with extinction and with
broadening against independent forms within the bounds table_los_support derives, the exact properties of the
statement, every refusal, and a ``problem.CurveProblem`` over a numpy scorer against the same run given the statement as
a plain model."""
import numpy as np
import pytest

from massivedatans_amd import _host, jointstate, problem, sample, tablemodel
from massivedatans_amd.tablemodel import BROADEN_CUT, TableModel
from chain_support import pow10_dd  # noqa: F401  (fixture)
from curves_support import NumpyFixedNoise
from oracle_backend import patch_neighbors
from table_support import EPS, abscissa, same_bits
from table_los_support import (bound_broadening, bound_extinction, dense_d, independent_broadening, independent_extinction,
                               longest_window, los_params, make_los_model, special_rows, window_s)


def test_host_pow10_dd_is_the_headers(pow10_dd):  # noqa: F811
    """libmdns_host.so's build of csrc/mdns_pow10.h equals the test build bit for bit: on the Gaussian's exponents
    [-5.5, 0], on the attenuation's [-299, 299], and at 0, where it is exactly 1."""
    rng = np.random.RandomState(1)
    for args in (np.linspace(-5.5, 0.0, 20001), rng.uniform(-5.5, 0.0, size=20000), np.linspace(-299.0, 299.0, 20001),
                 rng.uniform(-299.0, 299.0, size=20000), np.array([0.0, -0.0, 299.0, -299.0])):
        got, want = _host.pow10_dd(args), pow10_dd(args)
        assert got.shape == args.shape and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert _host.pow10_dd(np.array([0.0, -0.0])).tolist() == [1.0, 1.0]
    assert _host.pow10_dd(np.zeros((0,))).shape == (0,) and _host.pow10_dd(np.full((2, 3), 2.0)).tolist() == [[100.0] * 3] * 2


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_extinction_against_the_independent_form(d):
    """``A * numpy.interp(x / (1 + z), grid, template * 10.0 ** (ext * E))`` with the template blended axis by axis: all
    four combinations of z and A, E of both signs up to 3 (attenuations over seven decades)."""
    worst = 0.0
    for redshift in (False, True):
        for amplitude in (False, True):
            tm = make_los_model(d, seed=10 * d + 2 * redshift + amplitude, nw=60, redshift=redshift, amplitude=amplitude, broadening=False)
            assert tm.ndim == d + redshift + amplitude + 1 and tm.flags & 4 and not tm.flags & 8
            x = abscissa(tm, 200, seed=d)
            xs = los_params(tm, np.random.RandomState(d), 64, [], emax=3.0)
            got, want = tm.statement(x, xs), independent_extinction(tm, x, xs)
            assert got.shape == (64, 200) and np.isfinite(got).all()
            ratio = float((np.abs(got - want) / bound_extinction(tm, xs)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (d, redshift, amplitude, ratio)
    print("d=%d: worst |statement - independent| with extinction = %.3g of the bound" % (d, worst))
    assert worst > 0


BROADEN_SEEDS = {1: 11, 2: 12, 3: 13, 4: 14}


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_broadening_against_the_independent_form(d):
    """A dense row-normalised matrix of ``exp(-0.5 ((g_n / g_m - 1) / s)^2) * width`` applied with ``@``.  Preconditions
    of the bound, asserted: every table value positive, and no |d_mn| within 1e-9 of the cut (the seeds are fixed)."""
    worst = 0.0
    for redshift, amplitude in ((False, False), (True, True)):
        tm = make_los_model(d, seed=BROADEN_SEEDS[d] + redshift, nw=80, redshift=redshift, amplitude=amplitude, extinction=False, positive=True)
        assert (tm.table > 0).all() and tm.flags & 8 and not tm.flags & 4
        x = abscissa(tm, 150, seed=d)
        rng = np.random.RandomState(BROADEN_SEEDS[d])
        xs = los_params(tm, rng, 24, [0.0])
        xs[:, tm.at_s] = 10 ** rng.uniform(-3, -1, size=24)             # windows from a few knots to half the grid
        for s in xs[:, tm.at_s]:
            assert (np.abs(np.abs(dense_d(tm, s)) - BROADEN_CUT) > 1e-9).all(), s
        lengths = [longest_window(tm, s) for s in xs[:, tm.at_s]]
        assert min(lengths) <= 6 and max(lengths) >= 30, lengths
        got, want = tm.statement(x, xs), independent_broadening(tm, x, xs)
        assert np.isfinite(got).all() and (got > 0).all()
        ratio = float((np.abs(got - want) / bound_broadening(tm, xs)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (d, redshift, ratio)
    print("d=%d: worst |statement - independent| with broadening = %.3g of the bound" % (d, worst))
    assert worst > 0


def test_exact_properties_of_the_statement():
    tm = make_los_model(2, seed=5, lengths=[3, 4], nw=33)
    x = abscissa(tm, 41, seed=2)
    s0, s_one, s7, s_whole = window_s(tm)
    rng = np.random.RandomState(5)
    xs = los_params(tm, rng, 12, [s7])
    # s = 0: the same model built without the broadening, bit for bit (the route of either effect is one route)
    narrow = TableModel(tm.axes, tm.grid, tm.table, redshift=True, amplitude=True, extinction=tm.ext)
    at_zero = xs.copy()
    at_zero[:, tm.at_s] = 0.0
    assert same_bits(tm.statement(x, at_zero), narrow.statement(x, np.delete(at_zero, tm.at_s, axis=1)))
    # E = 0: the attenuation is exactly 1 -- the same model built without the extinction
    unreddened = TableModel(tm.axes, tm.grid, tm.table, redshift=True, amplitude=True, broadening=True)
    at_e0 = xs.copy()
    at_e0[:, tm.at_e] = 0.0
    assert same_bits(tm.statement(x, at_e0), unreddened.statement(x, np.delete(at_e0, tm.at_e, axis=1)))
    # every window {m}: R_m = (S_m K_m) / K_m, two rounded operations from S_m.  Read at the knots (t = 0: the curve
    # is R_k itself; the last knot is read at t = 1 from the cell before it and left out), no z, no A
    bare = TableModel(tm.axes, tm.grid, tm.table, extinction=tm.ext, broadening=True)
    rows = np.delete(np.delete(xs, -1, axis=1), tm.d, axis=1)
    rows[:, bare.at_s] = 0.0
    S = bare.statement(tm.grid, rows)[:, :-1]
    rows[:, bare.at_s] = s_one
    assert longest_window(tm, s_one) == 1
    R = bare.statement(tm.grid, rows)[:, :-1]
    assert (np.abs(R - S) <= 2 * EPS * (1 + 2 * EPS) * np.abs(S)).all() and not same_bits(R, S)
    # a constant template stays constant: every S_m is the same number sigma (the same operations), num = sum sigma K_n
    # with a rounding per product and L - 1 per sum, den L - 1, the quotient 1: R_m = sigma (1 + e), |e| <= 2 L eps,
    # where L is the window of m -- cut short at both ends of the grid.  The last knot, read at t = 1, adds the two
    # roundings of R_k + 1 * (R_k+1 - R_k): (2 L + 2) eps, with 1 % for the terms of second order
    flat = TableModel(tm.axes, tm.grid, np.full(tm.table.shape, 1.7), broadening=True)
    for s in (s_one, s7, s_whole):
        rows = np.column_stack((los_params(flat, rng, 5, [0.0])[:, :2], np.full(5, 0.0)))
        sigma = flat.statement(tm.grid, rows)
        assert (sigma == sigma[:, :1]).all()
        rows[:, -1] = s
        L = (np.abs(dense_d(tm, s)) <= BROADEN_CUT).sum(axis=1)
        assert L[0] < L[len(L) // 2] or s == s_one or s == s_whole                # (the ends are cut)
        R = flat.statement(tm.grid, rows)
        assert (np.abs(R - sigma) <= 1.01 * (2 * L[None, :] + 2) * EPS * sigma).all(), s
    # NaN rows: a NaN anywhere, E not finite, s < 0 or not finite -- those rows, and only they
    rows, names, first_nan = special_rows(tm, x)
    with np.errstate(all="ignore"):
        got = tm.statement(x, rows)
    assert np.isnan(got[first_nan:]).all() and not np.isnan(got[:first_nan]).any(), names
    assert len(rows) - first_nan == tm.ndim + 5
    with np.errstate(all="ignore"):
        assert same_bits(tm.statement(x, rows[::-1])[::-1], got) and same_bits(tm.statement(x, rows[3:4])[0], got[3])


def test_the_statement_without_the_effects_needs_no_library(monkeypatch):
    """With either effect the statement calls ``_host.pow10_dd`` and says so when the library is missing; without them
    it stays pure numpy."""
    tm = make_los_model(1, seed=2, nw=9)
    plain = TableModel(tm.axes, tm.grid, tm.table, redshift=True, amplitude=True)
    x = abscissa(tm, 7)
    want = plain.statement(x, np.array([[0.3, 0.1, 2.0]]))
    monkeypatch.setattr(_host, "_LIB", False)
    assert same_bits(plain.statement(x, np.array([[0.3, 0.1, 2.0]])), want)
    with pytest.raises(RuntimeError) as e:
        tm.statement(x, np.array([[0.3, 0.1, 0.2, 0.01, 2.0]]))
    assert "libmdns_host.so" in str(e.value)


def test_table_model_refusals(monkeypatch):
    axis, grid = np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0, 3.0, 5.0])
    table, ext = np.ones((3, 4)), np.array([0.1, 0.2, -0.3, 0.0])
    tm = TableModel([axis], grid, table, True, True, extinction=ext, broadening=True)
    assert tm.ndim == 5 and tm.flags == 15 and (tm.at_e, tm.at_s) == (2, 3)
    assert TableModel([axis], grid, table, extinction=ext).ndim == 2 and TableModel([axis], grid, table, broadening=True).flags == 8
    assert TableModel([axis], grid - 3.0, table, extinction=ext).flags == 4       # extinction alone takes any grid
    bad = [
        dict(extinction=ext[:3]),                                                # a wrong length
        dict(extinction=np.concatenate((ext, [0.0]))),
        dict(extinction=ext.reshape(2, 2)),
        dict(extinction=np.where(np.arange(4) == 1, np.nan, ext)),               # not finite
        dict(extinction=np.where(np.arange(4) == 3, -np.inf, ext)),
        dict(grid=grid - 1.0, broadening=True),                                  # grid[0] = 0
        dict(grid=grid - 2.5, broadening=True, extinction=ext),                  # grid[0] < 0
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            TableModel([axis], kw.pop("grid", grid), table, **kw)
    # more parameters than MDNS_MAX_DIM: four axes and four flags are 8, so the cap is lowered to meet it
    monkeypatch.setattr(tablemodel, "MAX_DIM", 4)
    assert TableModel([axis], grid, table, True, True, extinction=ext).ndim == 4
    with pytest.raises(ValueError) as e:
        TableModel([axis], grid, table, True, True, extinction=ext, broadening=True)
    assert "5 parameters" in str(e.value)
    for xs in (np.ones((2, 4)), np.ones((2, 6))):
        with pytest.raises(ValueError):
            tm.statement(grid, xs)


def _prior(tm, smax):
    lo = np.array([a[0] for a in tm.axes] + [0.0, -0.3, 0.0, -1.0])
    hi = np.array([a[-1] for a in tm.axes] + [0.1, 0.3, smax, 1.0])

    def priortransform_batch(us):
        xs = lo + (hi - lo) * np.asarray(us, dtype=float)
        xs[:, -1] = 10 ** xs[:, -1]
        return xs
    return priortransform_batch


def test_problem_and_model_file_refusals(tmp_path):
    tm = make_los_model(2, seed=1, lengths=[2, 3], nw=5)
    x = abscissa(tm, 8)
    y = np.zeros((8, 3))
    scorer = NumpyFixedNoise(y, 1.0)
    for ndim in (tm.ndim - 2, tm.ndim - 1, tm.ndim + 1):
        with pytest.raises(ValueError) as e:
            problem.CurveProblem(x, y, tm, _prior(tm, 0.01), ndim, backend=scorer)
        assert "table model" in str(e.value)
    assert problem.CurveProblem(x, y, tm, _prior(tm, 0.01), tm.ndim, backend=scorer).nparams == tm.ndim == 6
    text = """
import numpy
from massivedatans_amd.tablemodel import TableModel
model = TableModel([numpy.array([0.0, 1.0])], numpy.array([1.0, 2.0, 3.0]), numpy.ones((2, 3)), redshift=True,
                   extinction=numpy.array([-0.5, -0.4, -0.3]), broadening=True)
ndim = %s
def priortransform_batch(us):
    return numpy.asarray(us, dtype=float)
"""
    good = tmp_path / "table_ok.py"
    good.write_text(text % "4")
    got = sample.load_model(str(good))
    assert isinstance(got["model"], TableModel) and got["ndim"] == 4 and got["model"].flags == 13
    for value in ("2", "5"):
        wrong = tmp_path / "table_wrong.py"
        wrong.write_text(text % value)
        with pytest.raises(ValueError) as e:
            sample.load_model(str(wrong))
        assert "ndim" in str(e.value) and "takes 4" in str(e.value)


def test_problem_with_a_los_model_equals_its_statement_as_a_plain_model(oracle, monkeypatch):
    patch_neighbors(monkeypatch, oracle)
    tm = make_los_model(2, seed=7, lengths=[3, 4], nw=30)
    x = abscissa(tm, 40, seed=3, beyond=0.0)
    prior = _prior(tm, window_s(tm)[2])
    truth = prior(np.random.RandomState(1).uniform(0.2, 0.8, size=(6, tm.ndim)))
    y = np.ascontiguousarray((tm.statement(x, truth) + 0.05 * np.random.RandomState(2).normal(size=(6, 40))).T)
    runs = []
    for model in (tm, lambda xs: tm.statement(x, xs)):
        p = problem.CurveProblem(x, y, model, prior, tm.ndim, noise_level=0.05, backend=NumpyFixedNoise(y, 0.05))
        assert p.table is None
        sampler = sample.build_sampler(p, nlive_points=20, nsuperset_draws=10, use_graph=False, seed=1, fused=True)
        with np.errstate(all="ignore"):
            results = sample.integrate(sampler, 0.5, 0, 40)
        assert isinstance(sampler.joint, jointstate.HostJointState) and sampler.ndraws > 0
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert np.isfinite(runs[0][0]).all() and runs[0][2] == runs[1][2] and runs[0][3].shape[-1] == 6
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    # the non-draw path is the statement too
    p = problem.CurveProblem(x, y, tm, prior, tm.ndim, noise_level=0.05, backend=NumpyFixedNoise(y, 0.05))
    mask = np.array([True, False, True, True, False, True])
    assert np.array_equal(p.multi_loglikelihood_batch(truth, mask), NumpyFixedNoise(y, 0.05).loglike_batch(tm.statement(x, truth), mask))
