"""The table model's line-of-sight effects on the GPU (csrc/mdns_table.hip k_table_los_gather, k_table_los_blend,
k_table_los_broaden, k_table_los_resample; include/mdns.h Part 12): the kernels bit-equal to ``TableModel.statement``
around the tile of the template stages and of the channels, at the edges of the statement, a candidate's one value
through both entry points and across batches on one handle, draws against the curve draws of the statement under all
five curve statistics, a whole run, and the lifecycle and refusals of ``mdns_table_create_los``."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, MuseSpectra, WeightedSpectra
from massivedatans_amd.tablemodel import DeviceTable, TableModel
from curves_support import Chunks, gauss_prior, refused
from filter_support import _drive
from table_support import abscissa, dev_curves, same_bits
from table_los_support import TILE, los_params, make_los_model, special_rows, window_s

pytestmark = pytest.mark.gpu

# k_table_los_blend and k_table_los_broaden take TILE = 256 template knots per workgroup, the gather and the resampling
# TILE channels: one below, at and above it, two workgroups, the smallest grids
NW = (2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
NX = (1, TILE - 1, TILE, TILE + 1)
BS = (1, 2, 33)
# (d, axis lengths, nw, redshift, amplitude, extinction, broadening, nx, B): every d, every combination of the four flags
# with a new one among them, every nw, nx and B
CASES = [
    (1, [2], 2, False, False, True, False, 1, 1),
    (1, [7], TILE + 1, True, True, True, True, TILE - 1, 33),
    (1, [3], 3, False, False, False, True, TILE + 1, 2),
    (2, [2, 2], TILE - 1, False, True, True, True, TILE, 33),
    (2, [5, 2], TILE, True, False, False, True, 1, 33),
    (2, [2, 4], 2, True, True, False, True, TILE, 2),
    (3, [2, 3, 2], 2 * TILE + 1, False, False, True, True, TILE + 1, 33),
    (3, [4, 2, 5], TILE + 1, True, False, True, False, TILE - 1, 33),
    (3, [2, 2, 2], 3, False, True, False, True, TILE, 1),
    (4, [2, 2, 2, 2], TILE, True, True, True, False, TILE + 1, 2),
    (4, [3, 2, 4, 2], 2 * TILE + 1, False, True, True, False, 1, 33),
    (4, [2, 3, 2, 3], TILE - 1, True, False, True, True, TILE - 1, 33),
    (4, [3, 3, 2, 2], 3, True, True, True, True, TILE + 1, 33),
]


def test_the_cases_cover_every_size():
    flags = {c[3:7] for c in CASES}
    assert flags == {(z, a, e, s) for z in (False, True) for a in (False, True) for e in (False, True) for s in (False, True) if e or s}
    assert {c[0] for c in CASES} == {1, 2, 3, 4} and {c[2] for c in CASES} == set(NW) and {c[7] for c in CASES} == set(NX)
    assert {c[8] for c in CASES} == set(BS) and TILE == 256
    # the whole-grid window is asked for at nw <= TILE + 1 only
    assert any(c[6] and c[2] == TILE + 1 and c[8] == 33 for c in CASES)


def _s_values(tm):
    """0, windows {m}, about +-7 knots and -- on grids of TILE + 1 knots at most -- the whole grid."""
    return window_s(tm)[:4 if len(tm.grid) <= TILE + 1 else 3]


@pytest.mark.parametrize("d,lengths,nw,redshift,amplitude,extinction,broadening,nx,B", CASES)
def test_kernel_equals_the_statement(d, lengths, nw, redshift, amplitude, extinction, broadening, nx, B, hip):
    tm = make_los_model(d, seed=d * 100 + nw + nx, lengths=lengths, nw=nw, redshift=redshift, amplitude=amplitude,
                        extinction=extinction, broadening=broadening)
    assert tm.ndim == d + redshift + amplitude + extinction + broadening
    x = abscissa(tm, nx, seed=nx)
    xs = los_params(tm, np.random.RandomState(B + nw), B, _s_values(tm))
    if B >= 33:
        edges, _, _ = special_rows(tm, x)
        at = np.random.RandomState(B).choice(B, size=min(len(edges), 16), replace=False)
        xs[at] = edges[len(edges) - len(at):]                              # the NaN rows and their neighbours among them
    with np.errstate(all="ignore"):
        want = tm.statement(x, xs)
    table = tm.bind(x)
    assert hip.mdns_table_nparams(table.handle) == tm.ndim and hip.mdns_table_nx(table.handle) == nx
    got = table.curves(xs)
    assert got.shape == (B, nx) and same_bits(got, want)
    for pad in (0, 3):
        wide, untouched = dev_curves(hip, table, xs, pad)
        assert same_bits(wide, want) and untouched, pad
    table.close()


def _exact_clamp_model(d, seed, **kw):
    """A model whose ext holds +1.0 and -1.0 exactly at its first two knots: E = +-299 puts q exactly on the clamp."""
    tm = make_los_model(d, seed, **kw)
    ext = tm.ext.copy()
    ext[0], ext[1] = 1.0, -1.0
    return TableModel(tm.axes, tm.grid, tm.table, redshift=tm.redshift, amplitude=tm.amplitude, extinction=ext, broadening=tm.broadening)


@pytest.mark.parametrize("broadening", [False, True])
def test_edges_of_the_statement(broadening, hip):
    """q on and beyond +-299, every window size (cut at the first and at the last knot: the whole-grid one and every
    window of the end knots), s tiny and -0.0, u on the first, a middle and the last knot: the statement's bits.  E =
    +-inf, s < 0, s = +-inf, a NaN in each parameter in turn: the whole row NaN, and the other rows what they are
    without them."""
    tm = _exact_clamp_model(2, seed=41, lengths=[3, 2], nw=37, broadening=broadening)
    x = abscissa(tm, 33, seed=3)
    xs, names, first_nan = special_rows(tm, x)
    assert tm.ext[0] * 299.0 == 299.0 and tm.ext[1] * 299.0 == -299.0
    with np.errstate(all="ignore"):
        want = tm.statement(x, xs)
    table = tm.bind(x)
    got = table.curves(xs)
    for k, name in enumerate(names):
        assert same_bits(got[k], want[k]), name
    assert np.isnan(got[first_nan:]).all() and not np.isnan(got[:first_nan]).any(), names
    shuffled = np.random.RandomState(1).permutation(len(xs))
    assert same_bits(table.curves(xs[shuffled]), got[shuffled]) and same_bits(table.curves(xs[:first_nan]), got[:first_nan])
    # a template read at its own knots (the windows of the first and the last knot are cut by the ends of the grid)
    on_knots = tm.bind(tm.grid)
    rows = xs[:first_nan].copy()
    rows[:, tm.d] = 0.0                                                    # z = 0: u_j = grid[j]
    with np.errstate(all="ignore"):
        assert same_bits(on_knots.curves(rows), tm.statement(tm.grid, rows))
    on_knots.close()
    table.close()


def test_a_candidate_has_one_value(hip):
    """The same bits alone and at several places of batches of several sizes, through both entry points with rows of
    nx and of nx + 3 doubles (the padding untouched); then 33, 1 and 33 candidates again on one handle: a stale row of
    the grow-only S or R would show."""
    tm = make_los_model(3, seed=9, lengths=[4, 3, 5], nw=TILE + 44)
    x = abscissa(tm, TILE + 44, seed=9)
    rng = np.random.RandomState(9)
    s_values = window_s(tm)[:3]
    xs = los_params(tm, rng, 33, s_values)
    table = tm.bind(x)
    whole = table.curves(xs)
    with np.errstate(all="ignore"):
        assert same_bits(whole, tm.statement(x, xs))
    for k in (2, 17):                                                      # a +-7 window and a {m} one
        one = xs[k:k + 1]
        alone = table.curves(one)
        assert same_bits(alone[0], whole[k])
        for B, place in ((2, 1), (33, 0), (33, 32), (7, 3)):
            batch = los_params(tm, rng, B, s_values)
            batch[place] = one[0]
            assert same_bits(table.curves(batch)[place], alone[0]), (B, place)
            for pad in (0, 3):
                wide, untouched = dev_curves(hip, table, batch, pad)
                assert same_bits(wide[place], alone[0]) and untouched, (B, place, pad)
    other = los_params(tm, rng, 1, s_values[2:])
    with np.errstate(all="ignore"):
        want_other = tm.statement(x, other)
    assert same_bits(table.curves(xs), whole) and same_bits(table.curves(other), want_other) and same_bits(table.curves(xs), whole)
    table.close()


# ---- draws and a whole run ----
NXD, NDATA = 33, 70
STATS = ("noise", "marginal", "chi2", "poisson", "wstat")


def _positive_los_model(seed=2):
    """test_table_model._positive_model's table (positive templates over two axes) with z, E, s and A."""
    rng = np.random.RandomState(seed)
    a0, a1 = np.array([0.0, 0.3, 1.0, 1.6]), np.array([-1.0, 0.5, 1.0])
    grid = np.sort(np.concatenate(([350.0, 900.0], rng.uniform(350, 900, size=38))))
    width = (15.0 + 40.0 * a0)[:, None, None]
    table = 0.2 + (1.0 + 0.5 * a1[None, :, None]) * np.exp(-0.5 * ((grid[None, None, :] - 600.0) / width) ** 2)
    ext = -0.4 * (3.1 * (grid[0] / grid) ** 1.3 - 0.8)
    return TableModel([a0, a1], grid, table, redshift=True, amplitude=True, extinction=ext, broadening=True)


def _to_params(tm):
    """Rows of curves_support.gauss_prior as rows (p_0, p_1, z, E, s, A) of the model, all six from mu and log sigma
    alone (as test_table_model._to_params does): E in [-0.5, 0.5], s from 0 (every sixth) up to windows of +-7 knots."""
    a0, a1 = tm.axes
    s7 = window_s(tm)[2]

    def to_params(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        u1, u2 = (xs[:, 1] - 400.0) / 400.0, xs[:, 2] / 2.0
        u3, u4, u5, u6 = ((k * u1 + m * u2) % 1.0 for k, m in ((7.0, 3.0), (13.0, 5.0), (17.0, 11.0), (19.0, 23.0)))
        return np.ascontiguousarray(np.column_stack((a0[0] - 0.1 + (a0[-1] - a0[0] + 0.2) * u1, a1[0] - 0.1 + (a1[-1] - a1[0] + 0.2) * u2,
                                                     0.2 * u3, u5 - 0.5, np.where(u6 < 1.0 / 6, 0.0, s7 * u6), 0.5 * 100.0 ** u4)))
    return to_params


def _spectra(stat, tm, x):
    """NDATA spectra made from the model at parameters of its prior, for each of the five curve statistics."""
    rng = np.random.RandomState(5)
    truth = _to_params(tm)(gauss_prior(rng.uniform(size=(NDATA, 3))))
    clean = tm.statement(x, truth).T                                       # [nx, ndata]
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


@pytest.mark.parametrize("stat", STATS)
def test_draws_equal_curve_draws_of_the_statement(stat):
    """Two joint states on the same spectra, one given parameters (mdns_joint_init_table, mdns_backend_draw_table), one
    the statement's curves: live matrix after init, then prepare / draw / advance rounds with random row selections
    and a cut-down: accepted index, fill bits, thresholds, shelf sizes and live matrix, to the bit."""
    tm = _positive_los_model()
    x = np.linspace(420.0, 880.0, NXD)
    to_params = _to_params(tm)
    rng = np.random.RandomState(len(stat))
    spectra = _spectra(stat, tm, x)
    nlive = 12
    table = tm.bind(x)
    calls = []

    def statement(xs):
        calls.append(len(xs))
        with np.errstate(all="ignore"):
            return tm.statement(x, xs)
    dev = jointstate.CurveJointState(spectra, nlive, lambda xs: pytest.fail("the table state called a model"), shelf_cap=4, table=table)
    ref = jointstate.CurveJointState(spectra, nlive, statement, shelf_cap=4, ndim=tm.ndim)
    xs0 = to_params(gauss_prior(rng.uniform(size=(nlive, 3))))
    dev.init(xs0)
    ref.init(xs0)
    assert dev.nparams == tm.ndim == 6 and np.array_equal(dev.live_matrix(), ref.live_matrix()) and np.isfinite(dev.live_matrix()).all()
    ndraws = _drive(Chunks(dev, to_params, False), Chunks(ref, to_params, False), NDATA, rng, iterations=6, exact=True)
    assert ndraws > 0 and len(calls) > ndraws
    dev.close()
    ref.close()
    table.close()
    spectra.close()


def test_a_nan_row_is_never_accepted():
    """A NaN parameter, E = inf, s < 0 and s = inf: none of the five is ever the accepted candidate."""
    tm = _positive_los_model()
    x = np.linspace(420.0, 880.0, NXD)
    to_params = _to_params(tm)
    spectra = _spectra("chi2", tm, x)
    table = tm.bind(x)
    dev = jointstate.CurveJointState(spectra, 8, None, table=table)
    rng = np.random.RandomState(3)
    dev.init(to_params(gauss_prior(rng.uniform(size=(8, 3)))))
    dev.prepare()
    xs = to_params(gauss_prior(rng.uniform(size=(5, 3))))
    xs[0, 1], xs[1, tm.at_e], xs[2, tm.at_s], xs[3, tm.at_s], xs[4, tm.at_e] = np.nan, np.inf, -1e-3, np.inf, -np.inf
    assert np.isnan(table.curves(xs)).all()
    idx, _, _, n = dev.draw_params(xs, None)
    assert idx == -1 and n == 5
    dev.close()
    table.close()
    spectra.close()


def test_whole_run_equals_the_statement_as_a_plain_model():
    tm = _positive_los_model()
    x = np.linspace(420.0, 880.0, NXD)
    rng = np.random.RandomState(11)
    s7 = window_s(tm)[2]
    lo = np.array([tm.axes[0][0], tm.axes[1][0], 0.0, -0.3, 0.0, 0.5])
    hi = np.array([tm.axes[0][-1], tm.axes[1][-1], 0.2, 0.3, s7, 5.0])
    prior = lambda us: lo + (hi - lo) * np.asarray(us, dtype=float)       # one parameter per dimension of the cube
    truth = prior(rng.uniform(0.2, 0.8, size=(64, 6)))
    v = np.full((NXD, 64), 0.04)
    y = np.ascontiguousarray(tm.statement(x, truth).T + 0.2 * rng.normal(size=(NXD, 64)))
    called = []

    def plain(xs):
        called.append(len(xs))
        with np.errstate(all="ignore"):
            return tm.statement(x, xs)
    runs = []
    for model in (tm, plain):
        p = problem.CurveProblem(x, y, model, prior, tm.ndim, v=v, marginalise_scale=False)
        assert isinstance(p.backend, WeightedSpectra) and (p.table is not None) == (model is tm)
        if model is tm:
            fetched = []
            curves = p.table.curves
            p.model = lambda xs: (fetched.append(len(xs)), curves(xs))[1]
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=50, max_samples=60, use_graph=False, seed=1)
        assert type(sampler.joint).__name__ == "CurveJointState" and (sampler.joint.table is not None) == (model is tm)
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
        if model is tm:
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


def _raw_create_los(hip, x, axes, grid, table, flags, ext):
    n = np.array([len(a) for a in axes], dtype=np.int32)
    cat = np.ascontiguousarray(np.concatenate(axes), dtype=float)
    x, grid, table = (np.ascontiguousarray(a, dtype=float) for a in (x, grid, table))
    ext = None if ext is None else np.ascontiguousarray(ext, dtype=float)
    return hip.mdns_table_create_los(_lib.ptr(x), len(x), len(axes), _lib.ptr(n), _lib.ptr(cat), len(grid), _lib.ptr(grid), _lib.ptr(table),
                                     flags, _lib.opt(ext))


def test_create_and_destroy_with_and_without_use(hip):
    """Tables of 4 MB with both effects made and destroyed, unused and used (S and R grown), leave the free device
    memory where it was after the first cycle."""
    _lib.require_device()
    tm = make_los_model(2, seed=3, lengths=[16, 16], nw=2048)
    x = abscissa(tm, 200, seed=3)
    xs = los_params(tm, np.random.RandomState(3), 9, window_s(tm)[:3])
    with np.errstate(all="ignore"):
        want = tm.statement(x, xs)
    free = []
    for cycle in range(4):
        unused = tm.bind(x)
        used = DeviceTable(tm, x)
        assert same_bits(used.curves(xs), want) and dev_curves(hip, used, xs, 3)[1]
        unused.close()
        used.close()
        used.close()                                                       # (twice: nothing happens)
        with pytest.raises(_lib.MdnsError):
            used.curves(xs)
        free.append(_free_bytes())
    print("free device memory after the cycles: %s" % free)
    assert free[3] == free[1]


def test_refused_creates_leave_nothing_behind(hip):
    _lib.require_device()
    x, a, g = np.linspace(1.0, 2.0, 8), np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0, 3.0, 4.0])
    T, ext = np.ones((3, 4)), np.array([0.1, -0.2, 0.3, 0.0])
    E, S = _lib.TABLE_EXTINCTION, _lib.TABLE_BROADEN
    warm = _raw_create_los(hip, x, [a], g, T, E | S, ext)
    assert warm and hip.mdns_table_nparams(warm) == 3
    hip.mdns_table_destroy(warm)
    plain = _raw_create_los(hip, x, [a], g, T, 3, None)                    # neither new flag, no ext: mdns_table_create's case
    assert plain and hip.mdns_table_nparams(plain) == 3
    hip.mdns_table_destroy(plain)
    before = _free_bytes()
    bad_ext = ext.copy()
    bad_ext[2] = np.inf
    bad_T = T.copy()
    bad_T[2, 1] = np.nan
    cases = [
        (dict(grid=g, table=T, flags=E, ext=None), ("null ext",)),
        (dict(grid=g, table=T, flags=E | S, ext=bad_ext), ("ext[2]", "not finite")),
        (dict(grid=g, table=T, flags=E, ext=np.where(np.arange(4) == 0, np.nan, ext)), ("ext[0]", "not finite")),
        (dict(grid=g - 1.0, table=T, flags=S, ext=None), ("grid[0]", "MDNS_TABLE_BROADEN")),
        (dict(grid=g - 3.0, table=T, flags=E | S, ext=ext), ("grid[0]", "MDNS_TABLE_BROADEN")),
        (dict(grid=g, table=T, flags=16, ext=ext), ("flags=16", "unknown bits")),
        (dict(grid=g, table=T, flags=E | 32, ext=ext), ("flags=36", "unknown bits")),
        (dict(grid=g, table=bad_T, flags=E, ext=ext), ("table[9]", "not finite")),
        (dict(grid=np.array([1.0, 3.0, 2.0, 4.0]), table=T, flags=S, ext=None), ("grid", "[2]")),
    ]
    for kw, words in cases:
        h = _raw_create_los(hip, x, [a], **kw)
        assert not h, kw
        msg = _lib.last_error()
        assert "mdns_table_create_los" in msg and all(w in msg for w in words), (msg, words)
    # extinction alone takes a grid that is not positive; mdns_table_create still knows two flags only
    h = _raw_create_los(hip, x, [a], g - 3.0, T, E, ext)
    assert h
    hip.mdns_table_destroy(h)
    n1 = np.array([3], dtype=np.int32)
    assert not hip.mdns_table_create(_lib.ptr(x), 8, 1, _lib.ptr(n1), _lib.ptr(a), 4, _lib.ptr(g), _lib.ptr(T), 4)
    assert "mdns_table_create:" in _lib.last_error() and "flags=4" in _lib.last_error()
    assert _free_bytes() == before


def test_the_joint_entries_refuse_another_abscissa(hip):
    tm = _positive_los_model()
    x = np.linspace(420.0, 880.0, NXD)
    to_params = _to_params(tm)
    spectra = _spectra("noise", tm, x)
    table, other = tm.bind(x), tm.bind(x[:-1])
    xs = to_params(gauss_prior(np.random.RandomState(1).uniform(size=(8, 3))))
    js = jointstate.CurveJointState(spectra, 8, None, table=table)
    with pytest.raises(ValueError):
        jointstate.CurveJointState(spectra, 8, None, ndim=tm.ndim - 2, table=table)
    refused(hip.mdns_joint_init_table(js._h, other.handle, _lib.ptr(xs), 0.5, None), "mdns_joint_init_table", "%d channels" % (NXD - 1), "have %d" % NXD)
    js.init(xs)
    js.prepare()
    acc, nsc = C.c_int(7), C.c_int(0)
    bits = np.zeros((NDATA + 63) // 64, dtype=np.uint64)
    outs = (C.addressof(acc), _lib.ptr(bits), C.addressof(nsc))
    _lib.check(hip.mdns_backend_draw_begin(js._h, None, NDATA), "mdns_backend_draw_begin")
    refused(hip.mdns_backend_draw_table(js._h, other.handle, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_table", "%d channels" % (NXD - 1))
    js.close()
    table.close()
    other.close()
    spectra.close()
