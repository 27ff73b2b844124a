"""The sum model on the GPU (csrc/mdns_sum.hip k_sum_curves, include/mdns.h Part 14): the kernel bit-equal to
``SumModel.statement`` around its tile of 256 bins, for every kind of component and every way to attenuate, at the rows
of the rules; a candidate's one value through both entry points and across batches on one handle; draws against the curve
draws of the statement under all five curve statistics and under a response; a whole run; lifecycle and refusals."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, MuseSpectra, WeightedSpectra
from massivedatans_amd.response import Response
from massivedatans_amd.summodel import DeviceSum, GaussianLine, PowerLaw, SumModel
from curves_support import Chunks, gauss_prior, refused
from filter_support import _drive
from sum_support import (TILE, attenuation, dev_curves, edge_rows, los_table, model_params, positive_params, positive_prior, positive_sum,
                         rule_rows, table)
from table_support import same_bits

pytestmark = pytest.mark.gpu

# k_sum_curves takes TILE = 256 bins per workgroup: one below, at and above it (two workgroups), and a single bin
NX = (1, TILE - 1, TILE, TILE + 1)
BS = (1, 2, 33)
# (components, attenuation, nx, B).  Components: "pl", "g", ("t", d) a plain table over d axes, "bare" a plain table of
# one parameter, ("los", d, nw) a table with extinction and broadening (three kernels into its slice of the scratch).
# Attenuation: None, or which components the factor touches: "all", "none", "mixed" (every second one)
CASES = [
    (["pl"], None, 1, 1),
    (["g"], None, TILE - 1, 2),
    ([("t", 2)], None, TILE, 33),
    (["pl", "g", ("t", 1)], "all", TILE + 1, 33),
    (["pl", "g", "bare", "bare", "pl", "g", "bare", "bare"], "mixed", TILE + 1, 2),
    ([("t", 1), ("t", 3), "g"], "none", TILE - 1, 33),
    ([("los", 2, TILE - 1), "pl"], "mixed", TILE, 33),
    (["g", ("los", 1, TILE + 1), ("t", 2)], "all", 1, 33),
    ([("los", 1, TILE + 1), "g"], None, TILE + 1, 1),
]


def _kind(c):
    return c if isinstance(c, str) else c[0]


def test_the_cases_cover_every_size():
    assert {c[2] for c in CASES} == set(NX) and {c[3] for c in CASES} == set(BS) and TILE == 256
    alone = {_kind(c[0][0]) for c in CASES if len(c[0]) == 1}
    assert alone == {"pl", "g", "t"}
    assert any({"pl", "g", "t"} <= {_kind(k) for k in c[0]} for c in CASES)
    assert any(len(c[0]) == _lib.SUM_MAX_COMPONENTS for c in CASES)
    assert any(len({k[1] for k in c[0] if _kind(k) == "t"}) >= 2 for c in CASES)                 # two tables of different d
    assert {k[2] for c in CASES for k in c[0] if _kind(k) == "los"} == {TILE - 1, TILE + 1}      # nw on both sides of 256
    assert {c[1] for c in CASES} == {None, "all", "none", "mixed"}
    assert any(c[3] == 33 and c[1] is not None and {"pl", "g"} <= {_kind(k) for k in c[0]} for c in CASES)   # every rule is planted


def _abscissa(nx, seed):
    """``nx`` ascending positive bins that reach beyond both ends of the tables' grid (300 .. 900)."""
    if nx == 1:
        return np.array([600.0])
    return np.sort(np.random.RandomState(seed).uniform(280.0, 920.0, size=nx))


def _build(components, att, x, seed):
    made = []
    for k, c in enumerate(components):
        if c == "pl":
            made.append(PowerLaw(x0=500.0 + 20.0 * k))
        elif c == "g":
            made.append(GaussianLine())
        elif c == "bare":
            made.append(table(1, seed + k, redshift=False, amplitude=False))
        elif c[0] == "t":
            made.append(table(c[1], seed + k))
        else:
            made.append(los_table(c[1], seed + k, nw=c[2]))
    if att is None:
        return SumModel(made)
    free = {"all": [], "none": range(len(made)), "mixed": range(1, len(made), 2)}[att]
    return SumModel(made, attenuation=attenuation(x, seed), unattenuated=free)


@pytest.mark.parametrize("components,att,nx,B", CASES)
def test_kernel_equals_the_statement(components, att, nx, B, hip):
    x = _abscissa(nx, seed=nx)
    sm = _build(components, att, x, seed=nx + B)
    rng = np.random.RandomState(B + nx)
    xs = model_params(sm, x, rng, B)
    if B >= 33:
        rows = np.vstack((rule_rows(sm, x, xs[0])[0], edge_rows(sm, x, xs[1])[0]))
        at = rng.choice(np.arange(2, B), size=min(len(rows), 16), replace=False)
        xs[at] = rows[rng.choice(len(rows), size=len(at), replace=False)]
    with np.errstate(all="ignore"):
        want = sm.statement(x, xs)
    dsum = sm.bind(x)
    assert hip.mdns_sum_nparams(dsum.handle) == sm.ndim and hip.mdns_sum_nx(dsum.handle) == nx
    assert hip.mdns_sum_ncomponents(dsum.handle) == len(components)
    got = dsum.curves(xs)
    assert got.shape == (B, nx) and same_bits(got, want)
    for pad in (0, 3):
        wide, untouched = dev_curves(hip, dsum, xs, pad)
        assert same_bits(wide, want) and untouched, pad
    dsum.close()


@pytest.mark.parametrize("att", ["all", "mixed"])
def test_every_rule_and_edge_row(att, hip):
    """Every row of the rules (whole row NaN) and of the edges (no NaN from finite parameters) among good rows, in batches
    of 33: the statement's bits, and the good rows what they are alone."""
    x = _abscissa(40, seed=5)
    sm = _build(["pl", "g", ("t", 1), "g"], att, x, seed=9)
    good = model_params(sm, x, np.random.RandomState(3), 4, positive=True)
    bad, names = rule_rows(sm, x, good[0])
    edges, edge_names = edge_rows(sm, x, good[1])
    batch = np.vstack((good[:2], bad, good[2:], edges))
    with np.errstate(all="ignore"):
        want = sm.statement(x, batch)
    dsum = sm.bind(x)
    got = np.vstack([dsum.curves(batch[k:k + 33]) for k in range(0, len(batch), 33)])
    for k, name in enumerate(names + edge_names):
        row = 2 + k if k < len(bad) else 4 + k
        assert same_bits(got[row], want[row]) and np.isnan(got[row]).all() == (k < len(bad)), name
        assert np.isnan(got[row]).any() == (k < len(bad)), name
    assert same_bits(got, want) and same_bits(dsum.curves(good), got[[0, 1, 2 + len(bad), 3 + len(bad)]])
    dsum.close()


def test_exact_facts_on_the_device(hip):
    x = np.array([1.0, 2.0, 10.0, 17.5, 40.0])
    line = SumModel([GaussianLine()]).bind(x)
    got = line.curves([[3.7, 17.5, 2.0], [-0.3, 10.0, 1e-320]])
    assert got[0, 3] == 3.7 and got[1, 2] == -0.3 and not np.isnan(got).any() and (got[1, [0, 1, 3, 4]] == -0.3 * 1e-299).all()
    pl = SumModel([PowerLaw(x0=1.0)]).bind(x)
    assert (pl.curves([[0.0, 299.0], [0.0, 300.0]])[:, 2] == 1e-299).all()
    line.close()
    pl.close()
    # a lone table: the table's own curves, -0.0 become +0.0
    tm = table(2, 3)
    xt = _abscissa(50, 2)
    xs = model_params(SumModel([tm]), xt, np.random.RandomState(1), 6)
    xs[2, -1] = -0.0
    lone, own = SumModel([tm]).bind(xt), tm.bind(xt)
    mine, its = lone.curves(xs), own.curves(xs)
    assert np.signbit(its[2]).any() and not np.signbit(mine[2]).any() and same_bits(mine, its + 0.0)
    lone.close()
    own.close()


def test_a_candidate_has_one_value(hip):
    """The same bits alone and at places 0, 1 and 32 of batches of 2, 7 and 33, through both entry points with rows of nx
    and nx + 3 doubles (the padding untouched); then 33, 1 and 33 candidates again on one handle: a stale row of the
    grow-only scratch (the sum's, or the table's S and R) would show."""
    x = _abscissa(TILE + 44, seed=9)
    sm = _build([("los", 2, TILE + 44), "pl", ("t", 1), "g"], "mixed", x, seed=9)
    rng = np.random.RandomState(9)
    xs = model_params(sm, x, rng, 33)
    dsum = sm.bind(x)
    whole = dsum.curves(xs)
    with np.errstate(all="ignore"):
        assert same_bits(whole, sm.statement(x, xs))
    for k in (2, 17):
        one = xs[k:k + 1]
        alone = dsum.curves(one)
        assert same_bits(alone[0], whole[k])
        for B, place in ((2, 0), (2, 1), (7, 1), (33, 0), (33, 1), (33, 32)):
            batch = model_params(sm, x, rng, B)
            batch[place] = one[0]
            assert same_bits(dsum.curves(batch)[place], alone[0]), (B, place)
            for pad in (0, 3):
                wide, untouched = dev_curves(hip, dsum, batch, pad)
                assert same_bits(wide[place], alone[0]) and untouched, (B, place, pad)
    other = model_params(sm, x, rng, 1)
    with np.errstate(all="ignore"):
        want_other = sm.statement(x, other)
    assert same_bits(dsum.curves(xs), whole) and same_bits(dsum.curves(other), want_other) and same_bits(dsum.curves(xs), whole)
    dsum.close()


# ---- draws and a whole run ----
NXD, N_IN, NDATA = 33, 48, 70
STATS = ("noise", "marginal", "chi2", "poisson", "wstat")


def _spectra(stat, clean, x):
    """NDATA spectra made from the clean curves [nx, ndata], for each of the five curve statistics."""
    rng = np.random.RandomState(5)
    if stat == "noise":
        return GaussLineSpectra(x, clean + 0.5 * rng.normal(size=clean.shape), noise_level=0.5)
    v = rng.uniform(0.1, 0.5, size=clean.shape)
    y = clean + np.sqrt(v) * rng.normal(size=clean.shape)
    if stat == "marginal":
        return MuseSpectra(x, y, v)
    if stat == "chi2":
        return WeightedSpectra(x, y, v)
    e = rng.uniform(0.5, 2.0, size=clean.shape)
    n = rng.poisson(clean * e).astype(float)
    if stat == "poisson":
        return CountSpectra(x, n, e)
    g = rng.uniform(1.0, 3.0, size=clean.shape)
    return CountSpectra(x, n + rng.poisson(0.3 * e), e, rng.poisson(0.3 * g).astype(float), g)


def _banded_response():
    """33 channels x 48 bins: a band of positive entries around each channel's own bins (count rates stay >= 0)."""
    x, x_in = np.linspace(420.0, 880.0, NXD), np.linspace(420.0, 880.0, N_IN)
    centre = np.arange(NXD)[:, None] * (N_IN - 1.0) / (NXD - 1.0)
    R = np.exp(-0.5 * ((np.arange(N_IN)[None, :] - centre) / 1.2) ** 2)
    R[np.abs(np.arange(N_IN)[None, :] - centre) > 3.0] = 0.0
    return x, Response.from_dense(R / R.sum(axis=1, keepdims=True), x_in=x_in)


def _draw_states(stat, with_response):
    """``(dev, ref, to_params, closers)`` on the SAME spectra: one state handed parameters through the new entries with a
    model that fails if it is called, one handed the statement's curves."""
    if with_response:
        x, resp = _banded_response()
        model_x = resp.x_in
    else:
        x, resp, model_x = np.linspace(420.0, 880.0, NXD), None, np.linspace(420.0, 880.0, NXD)
    sm = positive_sum(model_x)
    to_params = positive_params(sm)
    truth = to_params(gauss_prior(np.random.RandomState(5).uniform(size=(NDATA, 3))))
    clean = sm.statement(model_x, truth)
    spectra = _spectra(stat, (clean if resp is None else resp.statement(clean)).T, x)
    if resp is not None:
        spectra.set_response(resp)
    dsum = sm.bind(model_x)
    calls = []

    def statement(xs):
        calls.append(len(xs))
        with np.errstate(all="ignore"):
            return sm.statement(model_x, xs)
    dev = jointstate.CurveJointState(spectra, 12, lambda xs: pytest.fail("the sum state called a model"), shelf_cap=4, table=dsum)
    ref = jointstate.CurveJointState(spectra, 12, statement, shelf_cap=4, ndim=sm.ndim)
    return dev, ref, to_params, calls, sm, (dev, ref, dsum, spectra)


@pytest.mark.parametrize("stat,with_response", [(s, False) for s in STATS] + [("poisson", True)])
def test_draws_equal_curve_draws_of_the_statement(stat, with_response):
    """Live matrix after init, then prepare / draw / advance rounds with random row selections and a cut-down: accepted
    index, fill bits, thresholds, shelf sizes and live matrix, to the bit."""
    dev, ref, to_params, calls, sm, closers = _draw_states(stat, with_response)
    rng = np.random.RandomState(len(stat))
    xs0 = to_params(gauss_prior(rng.uniform(size=(12, 3))))
    dev.init(xs0)
    ref.init(xs0)
    assert dev.nparams == sm.ndim == 10 and dev.n_in == (N_IN if with_response else NXD)
    assert np.array_equal(dev.live_matrix(), ref.live_matrix()) and np.isfinite(dev.live_matrix()).all()
    ndraws = _drive(Chunks(dev, to_params, False), Chunks(ref, to_params, False), NDATA, rng, iterations=6, exact=True)
    assert ndraws > 0 and len(calls) > ndraws
    for c in closers:
        c.close()


def test_a_nan_row_is_never_accepted():
    """A NaN parameter, sigma = 0 and N = inf: none is ever the accepted candidate."""
    dev, ref, to_params, _, sm, closers = _draw_states("chi2", False)
    rng = np.random.RandomState(3)
    dev.init(to_params(gauss_prior(rng.uniform(size=(12, 3)))))
    dev.prepare()
    xs = to_params(gauss_prior(rng.uniform(size=(3, 3))))
    xs[0, 6], xs[1, 4], xs[2, 9] = np.nan, 0.0, np.inf
    assert np.isnan(closers[2].curves(xs)).all()
    idx, _, _, n = dev.draw_params(xs, None)
    assert idx == -1 and n == 3
    for c in closers:
        c.close()


def test_whole_run_equals_the_statement_as_a_plain_model():
    x = np.linspace(420.0, 880.0, NXD)
    sm = positive_sum(x)
    prior = positive_prior(sm)
    rng = np.random.RandomState(11)
    truth = prior(rng.uniform(0.2, 0.8, size=(64, sm.ndim)))
    v = np.full((NXD, 64), 0.04)
    y = np.ascontiguousarray(sm.statement(x, truth).T + 0.2 * rng.normal(size=(NXD, 64)))
    called = []

    def plain(xs):
        called.append(len(xs))
        with np.errstate(all="ignore"):
            return sm.statement(x, xs)
    runs = []
    for model in (sm, plain):
        p = problem.CurveProblem(x, y, model, prior, sm.ndim, v=v, marginalise_scale=False)
        assert isinstance(p.backend, WeightedSpectra) and (p.table is not None) == (model is sm)
        if model is sm:
            assert isinstance(p.table, DeviceSum)
            fetched = []
            curves = p.table.curves
            p.model = lambda xs: (fetched.append(len(xs)), curves(xs))[1]
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=50, max_samples=60, use_graph=False, seed=1)
        assert type(sampler.joint).__name__ == "CurveJointState" and (sampler.joint.table is not None) == (model is sm)
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
        if model is sm:
            assert fetched == [], "curves were made through Python during the run"
        sampler.joint.close()
    assert called and runs[0][2] > 0 and runs[0][2] == runs[1][2] and np.isfinite(runs[0][0]).all()
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k


# ---- lifecycle and refusals ----
def _free_bytes():
    """Free device memory as the HIP runtime the library runs on reports it (hipMemGetInfo, behind a synchronise)."""
    lib = _lib.load()
    _lib.check(lib.mdns_sync(), "mdns_sync")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def test_create_and_destroy_with_and_without_use(hip):
    """Models with two tables of 2 MB (one on the broadening route), made and destroyed, unused and used (the scratch and
    the table's S and R grown), leave the free device memory where it was after the first cycle."""
    _lib.require_device()
    x = _abscissa(200, seed=3)
    sm = SumModel([los_table(2, 3, nw=1024, lengths=[16, 16]), PowerLaw(x0=500.0), table(2, 4, nw=1024, lengths=[16, 16]), GaussianLine()],
                  attenuation=attenuation(x), unattenuated=[3])
    xs = model_params(sm, x, np.random.RandomState(3), 9)
    with np.errstate(all="ignore"):
        want = sm.statement(x, xs)
    free = []
    for cycle in range(4):
        unused = sm.bind(x)
        used = DeviceSum(sm, x)
        assert same_bits(used.curves(xs), want) and dev_curves(hip, used, xs, 3)[1]
        unused.close()
        used.close()
        used.close()                                                       # (twice: nothing happens)
        with pytest.raises(_lib.MdnsError):
            used.curves(xs)
        free.append(_free_bytes())
    print("free device memory after the cycles: %s" % free)
    assert free[3] == free[1]


def _add_table(hip, h, T, flags=0, ext=None, grid=None, attenuated=1):
    a = np.array([0.0, 1.0, 2.0])
    g = np.array([1.0, 2.0, 3.0, 4.0]) if grid is None else np.ascontiguousarray(grid, dtype=float)
    n = np.array([3], dtype=np.int32)
    T = np.ascontiguousarray(T, dtype=float)
    ext = None if ext is None else np.ascontiguousarray(ext, dtype=float)
    return hip.mdns_sum_add_table(h, 1, _lib.ptr(n), _lib.ptr(a), 4, _lib.ptr(g), _lib.ptr(T), flags, _lib.opt(ext), attenuated)


def test_refusals_leave_the_model_as_it_was(hip):
    _lib.require_device()
    x = np.linspace(1.0, 2.0, 8)
    lx, att, T = np.log10(x), -0.1 * x, np.ones((3, 4))
    bad_x = x.copy()
    bad_x[5] = np.nan
    for args, words in (((None, 8), ("null argument",)), ((_lib.ptr(x), 0), ("nx=0",)), ((_lib.ptr(bad_x), 8), ("x[5]", "not finite"))):
        assert not hip.mdns_sum_create(*args)
        assert "mdns_sum_create" in _lib.last_error() and all(w in _lib.last_error() for w in words), _lib.last_error()
    # a warm-up model that goes through every add, so that nothing below is a first allocation of the process
    warm = hip.mdns_sum_create(_lib.ptr(x), 8)
    assert warm and _add_table(hip, warm, T, _lib.TABLE_EXTINCTION | _lib.TABLE_BROADEN, ext=att[:4]) == 0
    assert hip.mdns_sum_add_powerlaw(warm, _lib.ptr(lx), 1) == 0 and hip.mdns_sum_set_attenuation(warm, _lib.ptr(att)) == 0
    hip.mdns_sum_destroy(warm)
    h = hip.mdns_sum_create(_lib.ptr(x), 8)
    assert h and hip.mdns_sum_ncomponents(h) == 0 and hip.mdns_sum_nparams(h) == 0 and hip.mdns_sum_nx(h) == 8
    out, one = np.empty((1, 8)), np.ones((1, 16))
    refused(hip.mdns_sum_curves_batch(h, _lib.ptr(one), 1, _lib.ptr(out)), "mdns_sum_curves_batch", "without components")
    assert hip.mdns_sum_add_gauss(h, 1) == 0 and hip.mdns_sum_add_powerlaw(h, _lib.ptr(lx), 0) == 0 and _add_table(hip, h, T) == 0
    assert hip.mdns_sum_ncomponents(h) == 3 and hip.mdns_sum_nparams(h) == 6
    before = _free_bytes()
    bad_lx, bad_att, bad_T = lx.copy(), att.copy(), T.copy()
    bad_lx[2], bad_att[7], bad_T[2, 1] = np.inf, np.nan, np.nan
    E, S = _lib.TABLE_EXTINCTION, _lib.TABLE_BROADEN
    cases = [
        (lambda: hip.mdns_sum_add_powerlaw(h, None, 1), ("mdns_sum_add_powerlaw", "null argument")),
        (lambda: hip.mdns_sum_add_powerlaw(h, _lib.ptr(bad_lx), 1), ("mdns_sum_add_powerlaw", "lx[2]", "not finite")),
        (lambda: hip.mdns_sum_set_attenuation(h, None), ("mdns_sum_set_attenuation", "null argument")),
        (lambda: hip.mdns_sum_set_attenuation(h, _lib.ptr(bad_att)), ("mdns_sum_set_attenuation", "att[7]", "not finite")),
        (lambda: _add_table(hip, h, bad_T), ("mdns_sum_add_table", "table[9]", "not finite")),
        (lambda: _add_table(hip, h, T, E), ("mdns_sum_add_table", "null ext")),
        (lambda: _add_table(hip, h, T, 16), ("mdns_sum_add_table", "flags=16", "unknown bits")),
        (lambda: _add_table(hip, h, T, S, grid=[0.0, 1.0, 2.0, 3.0]), ("mdns_sum_add_table", "grid[0]", "MDNS_TABLE_BROADEN")),
        (lambda: hip.mdns_sum_add_gauss(None, 1), ("mdns_sum_add_gauss", "null sum handle")),
    ]
    for call, words in cases:
        refused(call(), *words)
        assert hip.mdns_sum_ncomponents(h) == 3 and hip.mdns_sum_nparams(h) == 6, words
    assert _free_bytes() == before
    # ndim above MDNS_MAX_DIM: 6 + 3 + 3 + 3 = 15, then a line (18), a power law (17), a table of 2 parameters (17)
    for k in range(3):
        assert hip.mdns_sum_add_gauss(h, k % 2) == 0
    for call, name, n in ((lambda: hip.mdns_sum_add_gauss(h, 1), "mdns_sum_add_gauss", 18), (lambda: hip.mdns_sum_add_powerlaw(h, _lib.ptr(lx), 1), "mdns_sum_add_powerlaw", 17),
                          (lambda: _add_table(hip, h, T, _lib.TABLE_AMPLITUDE), "mdns_sum_add_table", 17)):
        refused(call(), name, "%d parameters > 16" % n)
    assert hip.mdns_sum_set_attenuation(h, _lib.ptr(att)) == 0 and hip.mdns_sum_nparams(h) == 16 and hip.mdns_sum_ncomponents(h) == 6
    refused(hip.mdns_sum_set_attenuation(h, _lib.ptr(att)), "mdns_sum_set_attenuation", "attenuation already")
    # a ninth component: 8 bare tables hold 8 parameters
    many = hip.mdns_sum_create(_lib.ptr(x), 8)
    for k in range(8):
        assert _add_table(hip, many, T, attenuated=k % 2) == 0
    refused(_add_table(hip, many, T), "mdns_sum_add_table", "8 components at most")
    refused(hip.mdns_sum_add_gauss(many, 1), "mdns_sum_add_gauss", "8 components at most")
    assert hip.mdns_sum_ncomponents(many) == 8 and hip.mdns_sum_nparams(many) == 8
    # the first use fixes the model
    sm = SumModel([GaussianLine(), PowerLaw(x0=1.0), _as_table_model(T)] + [GaussianLine()] * 3, attenuation=att, unattenuated=[1, 3, 5])
    xs = model_params(sm, x, np.random.RandomState(1), 5)
    got = np.empty((5, 8))
    _lib.check(hip.mdns_sum_curves_batch(h, _lib.ptr(xs), 5, _lib.ptr(got)), "mdns_sum_curves_batch")
    with np.errstate(all="ignore"):
        assert same_bits(got, sm.statement(x, xs))
    ones, two = np.ones((2, 8)), np.empty((2, 8))
    _lib.check(hip.mdns_sum_curves_batch(many, _lib.ptr(ones), 2, _lib.ptr(two)), "mdns_sum_curves_batch")
    before = _free_bytes()
    for call, name in ((lambda: hip.mdns_sum_add_gauss(h, 1), "mdns_sum_add_gauss"), (lambda: hip.mdns_sum_add_powerlaw(h, _lib.ptr(lx), 1), "mdns_sum_add_powerlaw"),
                       (lambda: _add_table(hip, h, T), "mdns_sum_add_table"), (lambda: hip.mdns_sum_set_attenuation(many, _lib.ptr(att)), "mdns_sum_set_attenuation"),
                       (lambda: hip.mdns_sum_set_attenuation(h, _lib.ptr(att)), "mdns_sum_set_attenuation")):
        refused(call(), name, "the model is fixed at its first use")
    assert _free_bytes() == before and hip.mdns_sum_nparams(h) == 16 and hip.mdns_sum_nparams(many) == 8
    refused(hip.mdns_sum_curves_batch(h, _lib.ptr(xs), -1, _lib.ptr(got)), "mdns_sum_curves_batch", "bad sizes")
    refused(hip.mdns_sum_curves_batch(h, None, 2, _lib.ptr(got)), "mdns_sum_curves_batch", "null argument")
    refused(hip.mdns_sum_curves_batch_dev(h, _lib.ptr(xs), 2, _lib.ptr(got), 7), "mdns_sum_curves_batch_dev", "ldc=7")
    _lib.check(hip.mdns_sum_curves_batch(h, _lib.ptr(xs), 5, _lib.ptr(got)), "mdns_sum_curves_batch")
    with np.errstate(all="ignore"):
        assert same_bits(got, sm.statement(x, xs))
    hip.mdns_sum_destroy(h)
    hip.mdns_sum_destroy(many)
    hip.mdns_sum_destroy(None)


def _as_table_model(T):
    """``_add_table``'s table as a TableModel."""
    from massivedatans_amd.tablemodel import TableModel
    return TableModel([np.array([0.0, 1.0, 2.0])], np.array([1.0, 2.0, 3.0, 4.0]), T)


def test_the_joint_entries_refuse_another_abscissa_and_an_empty_model(hip):
    dev, ref, to_params, _, sm, closers = _draw_states("noise", False)
    x = np.linspace(420.0, 880.0, NXD)
    other = positive_sum(x[:-1]).bind(x[:-1])
    empty = hip.mdns_sum_create(_lib.ptr(x), NXD)
    xs = to_params(gauss_prior(np.random.RandomState(1).uniform(size=(12, 3))))
    with pytest.raises(ValueError):
        jointstate.CurveJointState(closers[3], 12, None, ndim=sm.ndim - 2, table=closers[2])
    refused(hip.mdns_joint_init_sum(dev._h, other.handle, _lib.ptr(xs), 0.5, None), "mdns_joint_init_sum", "%d channels" % (NXD - 1), "have %d" % NXD)
    refused(hip.mdns_joint_init_sum(dev._h, empty, _lib.ptr(xs), 0.5, None), "mdns_joint_init_sum", "without components")
    refused(hip.mdns_joint_init_sum(dev._h, None, _lib.ptr(xs), 0.5, None), "mdns_joint_init_sum", "null sum handle")
    dev.init(xs)
    dev.prepare()
    acc, nsc = C.c_int(7), C.c_int(0)
    bits = np.zeros((NDATA + 63) // 64, dtype=np.uint64)
    outs = (C.addressof(acc), _lib.ptr(bits), C.addressof(nsc))
    _lib.check(hip.mdns_backend_draw_begin(dev._h, None, NDATA), "mdns_backend_draw_begin")
    refused(hip.mdns_backend_draw_sum(dev._h, other.handle, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_sum", "%d channels" % (NXD - 1))
    refused(hip.mdns_backend_draw_sum(dev._h, empty, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_sum", "without components")
    assert acc.value == -1
    # the refused model is still open: it was never used
    assert hip.mdns_sum_add_gauss(empty, 1) == 0 and hip.mdns_sum_ncomponents(empty) == 1
    hip.mdns_sum_destroy(empty)
    other.close()
    for c in closers:
        c.close()


def test_under_a_response_the_entries_want_its_bins(hip):
    dev, ref, to_params, _, sm, closers = _draw_states("poisson", True)
    x = np.linspace(420.0, 880.0, NXD)
    on_channels = positive_sum(x).bind(x)
    xs = to_params(gauss_prior(np.random.RandomState(1).uniform(size=(12, 3))))
    refused(hip.mdns_joint_init_sum(dev._h, on_channels.handle, _lib.ptr(xs), 0.5, None), "mdns_joint_init_sum", "%d bins" % NXD, "takes %d" % N_IN)
    on_channels.close()
    for c in closers:
        c.close()
