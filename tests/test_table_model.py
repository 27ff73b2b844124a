"""The table model on the GPU (csrc/mdns_table.hip k_table_curves, include/mdns.h Part 12): the kernel bit-equal to
``TableModel.statement`` at the edges of its tile and of the statement, a candidate's one value, draws and initial
points through ``mdns_backend_draw_table`` / ``mdns_joint_init_table`` against ``mdns_backend_draw_curves`` /
``mdns_joint_init_curves`` fed with the statement's curves under all five curve statistics, a whole run, and the
handle's lifecycle and refusals."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, MuseSpectra, WeightedSpectra
from massivedatans_amd.tablemodel import DeviceTable, TableModel
from curves_support import Chunks, gauss_prior, refused
from filter_support import _drive
from table_support import TILE, abscissa, dev_curves, edge_params, make_model, random_params, same_bits

pytestmark = pytest.mark.gpu

# k_table_curves writes TILE = 256 channels per workgroup: one below, at and above it, one channel, and the 200 of the bench
NX = (1, TILE - 1, TILE, TILE + 1, 200)
BS = (1, 2, 33, 1024)
NW = (2, 3, 257)
# (d, axis lengths, nw, redshift, amplitude, nx, B): every d, every flag combination, axes of 2 knots, every nw, nx, B
CASES = [
    (1, [2], 2, False, False, 1, 1),
    (1, [7], 257, True, True, TILE - 1, 33),
    (1, [3], 3, True, False, TILE + 1, 1024),
    (2, [2, 2], 3, False, True, TILE, 2),
    (2, [5, 2], 257, True, True, 200, 1024),
    (2, [2, 4], 2, True, False, TILE + 1, 33),
    (3, [2, 3, 2], 257, False, False, TILE - 1, 2),
    (3, [4, 2, 5], 3, True, True, 200, 33),
    (3, [2, 2, 2], 2, False, True, TILE, 1024),
    (4, [2, 2, 2, 2], 2, True, True, 1, 33),
    (4, [3, 2, 4, 2], 257, True, False, TILE + 1, 1),
    (4, [2, 3, 2, 3], 3, False, True, 200, 2),
    (4, [3, 3, 2, 2], 257, True, True, 2 * TILE + 1, 1024),
]


def test_the_cases_cover_every_size():
    assert {c[0] for c in CASES} == {1, 2, 3, 4} and {(c[3], c[4]) for c in CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c[2] for c in CASES} == set(NW) and {c[5] for c in CASES} >= set(NX) and {c[6] for c in CASES} == set(BS)
    assert all(2 in c[1] for c in CASES if c[0] > 1) and TILE == 256


def _mixed(tm, x, B, seed):
    """``B`` candidates: random ones, inside and outside the axes, with the edge rows of the statement among them where
    they fit (the rows with a NaN last)."""
    xs = random_params(tm, np.random.RandomState(seed), B)
    edges, _, _ = edge_params(tm, x)
    n = min(len(edges), B // 2)
    at = np.random.RandomState(seed + 1).choice(B, size=n, replace=False)
    xs[at] = edges[len(edges) - n:]
    return xs


@pytest.mark.parametrize("d,lengths,nw,redshift,amplitude,nx,B", CASES)
def test_kernel_equals_the_statement(d, lengths, nw, redshift, amplitude, nx, B, hip):
    tm = make_model(d, seed=d * 100 + nw + nx, lengths=lengths, nw=nw, redshift=redshift, amplitude=amplitude)
    x = abscissa(tm, nx, seed=nx)
    xs = _mixed(tm, x, B, seed=B)
    with np.errstate(all="ignore"):
        want = tm.statement(x, xs)
    table = tm.bind(x)
    assert hip.mdns_table_nparams(table.handle) == tm.ndim and hip.mdns_table_nx(table.handle) == nx
    got = table.curves(xs)
    assert got.shape == (B, nx) and same_bits(got, want)
    for pad in (0, 1, 7):
        wide, untouched = dev_curves(hip, table, xs, pad)
        assert same_bits(wide, want) and untouched, pad
    table.close()


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_edges_of_the_statement(d, hip):
    """Parameters on every knot (first and last included), outside the axes, +-inf, u on grid knots, below grid[0] and
    above grid[-1], z = -1, +-inf in z and A: the statement's bits.  A NaN in any one parameter: the whole row NaN, and
    the other rows what they are without it."""
    tm = make_model(d, seed=40 + d, lengths=[3, 2, 4, 2][:d], nw=9)
    x = abscissa(tm, 33, seed=d)
    xs, names, first_nan = edge_params(tm, x)
    with np.errstate(all="ignore"):
        want = tm.statement(x, xs)
    table = tm.bind(x)
    got = table.curves(xs)
    for k, name in enumerate(names):
        assert same_bits(got[k], want[k]), name
    assert np.isnan(got[first_nan:]).all() and not np.isnan(got[:first_nan]).all(axis=1).any()
    # the neighbours of a NaN row are what they are without it
    mixed = []
    for k in range(first_nan):                                             # a NaN row behind each of the first rows
        mixed.append(k)
        if k < tm.ndim:
            mixed.append(first_nan + k)
    mixed = np.array(mixed)
    shuffled = np.random.RandomState(d).permutation(len(xs))
    assert same_bits(table.curves(xs[shuffled]), got[shuffled]) and same_bits(table.curves(xs[mixed]), got[mixed])
    assert same_bits(table.curves(xs[:first_nan]), got[:first_nan])
    # x = 0 under z = -1 is 0 / 0: that channel alone is NaN, on both sides
    if tm.redshift:
        x0 = np.concatenate(([0.0], x))
        t0 = tm.bind(x0)
        row = np.array([[0.5 * (a[0] + a[1]) for a in tm.axes] + [-1.0] + ([2.0] if tm.amplitude else [])])
        with np.errstate(all="ignore"):
            w0 = tm.statement(x0, row)
        g0 = t0.curves(row)
        assert same_bits(g0, w0) and np.isnan(g0[0, 0]) and np.isfinite(g0[0, 1:]).all()
        t0.close()
    table.close()


def test_a_candidate_has_one_value(hip):
    """The same bits alone, at several places of a batch of 1024, in a permuted batch, and through both entry points
    with several row strides."""
    tm = make_model(3, seed=9, lengths=[4, 3, 5], nw=64)
    x = abscissa(tm, TILE + 44, seed=9)
    rng = np.random.RandomState(9)
    xs = random_params(tm, rng, 1024)
    table = tm.bind(x)
    whole = table.curves(xs)
    with np.errstate(all="ignore"):
        assert same_bits(whole, tm.statement(x, xs))
    one = xs[17:18]
    alone = table.curves(one)
    assert same_bits(alone[0], whole[17])
    for place in (0, 1, 63, 64, 511, 1023):
        batch = xs.copy()
        batch[place] = one[0]
        assert same_bits(table.curves(batch)[place], alone[0]), place
        assert same_bits(dev_curves(hip, table, batch, 3)[0][place], alone[0]), place
    perm = rng.permutation(1024)
    assert same_bits(table.curves(xs[perm]), whole[perm])
    for pad in (0, 5, 56):
        assert same_bits(dev_curves(hip, table, one, pad)[0], alone), pad
    table.close()


# ---- draws and initial points under the five curve statistics ----
NXD, NDATA = 33, 70


def _positive_model(seed=2):
    """A table of positive templates (count rates must be >= 0) over two axes, with z and A."""
    rng = np.random.RandomState(seed)
    a0, a1 = np.array([0.0, 0.3, 1.0, 1.6]), np.array([-1.0, 0.5, 1.0])
    grid = np.sort(np.concatenate(([350.0, 900.0], rng.uniform(350, 900, size=38))))
    width = (15.0 + 40.0 * a0)[:, None, None]
    table = 0.2 + (1.0 + 0.5 * a1[None, :, None]) * np.exp(-0.5 * ((grid[None, None, :] - 600.0) / width) ** 2)
    return TableModel([a0, a1], grid, table, redshift=True, amplitude=True)


def _to_params(tm):
    """Rows of curves_support.gauss_prior (A, mu in [400, 800], log sigma in [0, 2]) as rows of the table model: the two
    axes overreached a little, z in [0, 0.2], A in [0.5, 50] -- all four from mu and log sigma alone, so that the faint
    lines filter_support._drive turns to after a few passes (small A) stay draws from the whole prior."""
    a0, a1 = tm.axes

    def to_params(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        u1, u2 = (xs[:, 1] - 400.0) / 400.0, xs[:, 2] / 2.0
        u3, u4 = (7.0 * u1 + 3.0 * u2) % 1.0, (13.0 * u1 + 5.0 * u2) % 1.0
        return np.ascontiguousarray(np.column_stack((a0[0] - 0.1 + (a0[-1] - a0[0] + 0.2) * u1, a1[0] - 0.1 + (a1[-1] - a1[0] + 0.2) * u2,
                                                     0.2 * u3, 0.5 * 100.0 ** u4)))
    return to_params


def _spectra(stat, tm, x):
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


STATS = ("noise", "marginal", "chi2", "poisson", "wstat")


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("stat", STATS)
def test_draws_equal_curve_draws_of_the_statement(stat, noisy):
    """Two joint states on the same spectra, one given parameters (mdns_joint_init_table, mdns_backend_draw_table), one
    the statement's curves (mdns_joint_init_curves, mdns_backend_draw_curves): live matrix after init -- with and
    without jitter --, then over prepare / draw / advance rounds with random row selections, a cut-down and -- noisy --
    a jitter block per chunk: accepted index, fill bits, thresholds, shelf sizes and live matrix, to the bit."""
    tm = _positive_model()
    x = np.linspace(420.0, 880.0, NXD)
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
    rng = np.random.RandomState(len(stat) + 7 * noisy)
    to_params = _to_params(tm)
    xs0 = to_params(gauss_prior(rng.uniform(size=(nlive, 3))))
    noise0 = rng.normal(0, 1e-5, size=(nlive, NDATA)) if noisy else None
    dev.init(xs0, jitter=noise0)
    ref.init(xs0, jitter=noise0)
    assert dev.nparams == tm.ndim and np.array_equal(dev.live_matrix(), ref.live_matrix()) and np.isfinite(dev.live_matrix()).all()
    ndraws = _drive(Chunks(dev, to_params, noisy), Chunks(ref, to_params, noisy), NDATA, rng, iterations=6, exact=True)
    assert ndraws > 0 and len(calls) > ndraws
    dev.close()
    ref.close()
    table.close()
    spectra.close()


def test_a_nan_candidate_is_never_accepted():
    tm = _positive_model()
    x = np.linspace(420.0, 880.0, NXD)
    spectra = _spectra("chi2", tm, x)
    table = tm.bind(x)
    dev = jointstate.CurveJointState(spectra, 8, None, table=table)
    rng = np.random.RandomState(3)
    to_params = _to_params(tm)
    dev.init(to_params(gauss_prior(rng.uniform(size=(8, 3)))))
    dev.prepare()
    xs = to_params(gauss_prior(rng.uniform(size=(5, 3))))
    xs[:, 1] = np.nan
    idx, _, _, n = dev.draw_params(xs, None)
    assert idx == -1 and n == 5
    dev.close()
    table.close()
    spectra.close()


def test_whole_run_equals_the_statement_as_a_plain_model():
    tm = _positive_model()
    x = np.linspace(420.0, 880.0, NXD)
    rng = np.random.RandomState(11)
    lo = np.array([tm.axes[0][0], tm.axes[1][0], 0.0, 0.5])
    hi = np.array([tm.axes[0][-1], tm.axes[1][-1], 0.2, 5.0])
    prior = lambda us: lo + (hi - lo) * np.asarray(us, dtype=float)       # one parameter per dimension of the cube
    truth = prior(rng.uniform(0.2, 0.8, size=(64, 4)))
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
            # the non-draw path fetches the device's curves: the statement's bits, scored like any other curves
            L = p.multi_loglikelihood_batch(truth[:5], np.ones(64, dtype=bool))
            assert fetched == [5] and np.array_equal(L, p.backend.loglike_batch_curves(tm.statement(x, truth[:5])))
        sampler.joint.close()
    assert called and runs[0][2] > 0 and runs[0][2] == runs[1][2] and np.isfinite(runs[0][0]).all()
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k


# ---- lifecycle and refusals ----
def _free_bytes():
    """Free device memory as the HIP runtime the library runs on reports it (hipMemGetInfo, behind a synchronise).  The
    symbol is looked up through the library's own handle, which searches its dependencies: the runtime it is linked
    to, whatever other copy a process may have mapped beside it."""
    lib = _lib.load()
    _lib.check(lib.mdns_sync(), "mdns_sync")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def _raw_create(hip, x, axes, grid, table, flags=0, d=None, n=None, nw=None, nx=None):
    n = np.array([len(a) for a in axes] if n is None else n, dtype=np.int32)
    cat = np.ascontiguousarray(np.concatenate(axes), dtype=float)
    x, grid, table = (np.ascontiguousarray(a, dtype=float) for a in (x, grid, table))
    return hip.mdns_table_create(_lib.ptr(x), len(x) if nx is None else nx, len(axes) if d is None else d, _lib.ptr(n), _lib.ptr(cat),
                                 len(grid) if nw is None else nw, _lib.ptr(grid), _lib.ptr(table), flags)


def test_create_and_destroy_with_and_without_use(hip):
    """Tables of 8 MB made and destroyed, unused and used, leave the free device memory where it was after the first
    cycle (which makes what lives as long as the process); a destroyed handle's wrapper says so."""
    _lib.require_device()
    tm = make_model(2, seed=3, lengths=[32, 16], nw=2048)
    x = abscissa(tm, 200, seed=3)
    xs = random_params(tm, np.random.RandomState(3), 33)
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
    hip.mdns_table_destroy(None)
    assert hip.mdns_table_nparams(None) == -1 and hip.mdns_table_nx(None) == -1


def test_refused_creates_leave_nothing_behind(hip):
    _lib.require_device()
    x, a, g = np.linspace(1.0, 2.0, 8), np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0, 3.0, 4.0])
    T = np.ones((3, 4))
    warm = _raw_create(hip, x, [a], g, T)
    assert warm
    hip.mdns_table_destroy(warm)
    before = _free_bytes()
    bad_T = T.copy()
    bad_T[2, 1] = np.nan
    cases = [
        (dict(x=x, axes=[a], grid=g, table=T, d=0), ("d=0",)),
        (dict(x=x, axes=[a], grid=g, table=T, d=5), ("d=5",)),
        (dict(x=x, axes=[a], grid=g, table=T, nx=0), ("nx=0",)),
        (dict(x=x, axes=[a], grid=g, table=T, nx=(1 << 20) + 1), ("nx=",)),
        (dict(x=x, axes=[a], grid=g, table=T, nw=1), ("nw=1",)),
        (dict(x=x, axes=[a], grid=g, table=T, n=[1]), ("axis 0", "1 knots")),
        (dict(x=x, axes=[a], grid=g, table=T, flags=4), ("flags=4",)),
        (dict(x=x, axes=[a[::-1]], grid=g, table=T), ("axis 0", "strictly increasing")),
        (dict(x=x, axes=[np.array([0.0, 1.0, 1.0])], grid=g, table=T), ("axis 0", "knot 2")),
        (dict(x=x, axes=[np.array([0.0, np.inf, 2.0])], grid=g, table=T), ("axis 0", "knot 1", "not finite")),
        (dict(x=x, axes=[a], grid=np.array([1.0, 3.0, 2.0, 4.0]), table=T), ("grid", "[2]")),
        (dict(x=x, axes=[a], grid=np.array([1.0, 2.0, 3.0, np.nan]), table=T), ("grid[3]", "not finite")),
        (dict(x=x, axes=[a], grid=g, table=bad_T), ("table[9]", "not finite")),
        (dict(x=np.where(np.arange(8) == 5, np.inf, x), axes=[a], grid=g, table=T), ("x[5]", "not finite")),
        # sizes whose product leaves int indexing: four axes of 2**15 knots are never read (the size test comes first)
        (dict(x=x, axes=[a, a, a, a], grid=g, table=T, n=[1 << 15] * 4), ("too large",)),
    ]
    for kw, words in cases:
        h = _raw_create(hip, **kw)
        assert not h, kw
        msg = _lib.last_error()
        assert "mdns_table_create" in msg and all(w in msg for w in words), (msg, words)
    n1 = np.array([3], dtype=np.int32)
    assert not hip.mdns_table_create(None, 8, 1, _lib.ptr(n1), _lib.ptr(a), 4, _lib.ptr(g), _lib.ptr(T), 0) and "null argument" in _lib.last_error()
    assert not hip.mdns_table_create(_lib.ptr(x), 8, 1, _lib.ptr(n1), _lib.ptr(a), 4, _lib.ptr(g), None, 0) and "null argument" in _lib.last_error()
    assert _free_bytes() == before
    # the Python class refuses the same before any device call
    with pytest.raises(ValueError):
        TableModel([a], g, bad_T)


def test_batch_and_joint_refusals(hip):
    tm = _positive_model()
    x = np.linspace(420.0, 880.0, NXD)
    spectra = _spectra("noise", tm, x)
    table = tm.bind(x)
    other = tm.bind(x[:-1])                                                # a table for another abscissa
    xs = _to_params(tm)(gauss_prior(np.random.RandomState(1).uniform(size=(8, 3))))
    out = np.empty((8, NXD))
    # the batch entries
    refused(hip.mdns_table_curves_batch(None, _lib.ptr(xs), 8, _lib.ptr(out)), "mdns_table_curves_batch", "null table")
    refused(hip.mdns_table_curves_batch(table.handle, _lib.ptr(xs), -1, _lib.ptr(out)), "mdns_table_curves_batch", "B=-1")
    refused(hip.mdns_table_curves_batch(table.handle, None, 8, _lib.ptr(out)), "mdns_table_curves_batch", "null argument")
    assert hip.mdns_table_curves_batch(table.handle, None, 0, None) == 0
    d_p, d_o = hip.mdns_dev_alloc(xs.nbytes), hip.mdns_dev_alloc(out.nbytes)
    refused(hip.mdns_table_curves_batch_dev(table.handle, d_p, 8, d_o, NXD - 1), "mdns_table_curves_batch_dev", "ldc=%d" % (NXD - 1), "nx=%d" % NXD)
    refused(hip.mdns_table_curves_batch_dev(table.handle, d_p, 8, None, NXD), "mdns_table_curves_batch_dev", "null argument")
    assert hip.mdns_table_curves_batch_dev(table.handle, d_p, 0, d_o, NXD) == 0
    hip.mdns_dev_free(d_p)
    hip.mdns_dev_free(d_o)
    with pytest.raises(ValueError):
        table.curves(xs[:, :3])
    # the joint entries
    js = jointstate.CurveJointState(spectra, 8, None, table=table)
    with pytest.raises(ValueError):
        jointstate.CurveJointState(spectra, 8, None, ndim=tm.ndim + 1, table=table)
    refused(hip.mdns_joint_init_table(js._h, other.handle, _lib.ptr(xs), 0.5, None), "mdns_joint_init_table", "%d channels" % (NXD - 1), "have %d" % NXD)
    refused(hip.mdns_joint_init_table(js._h, None, _lib.ptr(xs), 0.5, None), "mdns_joint_init_table", "null table")
    js.init(xs)
    live = js.live_matrix()
    js.prepare()
    acc, nsc = C.c_int(7), C.c_int(0)
    bits = np.zeros((NDATA + 63) // 64, dtype=np.uint64)
    outs = (C.addressof(acc), _lib.ptr(bits), C.addressof(nsc))
    refused(hip.mdns_backend_draw_table(js._h, table.handle, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_table", "no draw begun")
    assert acc.value == -1
    _lib.check(hip.mdns_backend_draw_begin(js._h, None, NDATA), "mdns_backend_draw_begin")
    refused(hip.mdns_backend_draw_table(js._h, other.handle, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_table", "%d channels" % (NXD - 1))
    refused(hip.mdns_backend_draw_table(js._h, None, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_table", "null table")
    # more candidates than MDNS_JOINT_MAX_BATCH: the rule of the curve entries -- the ABI refuses, the class looks at the first 1024
    many = np.ascontiguousarray(np.tile(xs, (130, 1)))
    assert len(many) == 1040
    refused(hip.mdns_backend_draw_table(js._h, table.handle, _lib.ptr(many), 1040, None, *outs), "mdns_backend_draw_table", "B=1040", "<= 1024")
    curves = np.empty((1040, NXD))
    refused(hip.mdns_backend_draw_curves(js._h, _lib.ptr(curves), 1040, None, *outs), "mdns_backend_draw_curves", "B=1040", "<= 1024")
    assert hip.mdns_backend_draw_table(js._h, table.handle, _lib.ptr(xs), 0, None, *outs) == 0 and acc.value == -1 and nsc.value == 0
    assert np.array_equal(js.live_matrix(), live)                          # nothing of it touched the state
    idx, _, beats, n = js.draw_params(many, None)
    assert n == 1024 and idx >= 0 and beats.any()
    js.close()
    for h in (table, other):
        h.close()
    spectra.close()
