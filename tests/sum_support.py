"""Test helper for the sum model (tests/test_sum_model_host.py, tests/test_sum_model.py): models of every kind of
component, their parameters, the INDEPENDENT forms -- ``10**logA * (x/x0)**-G``, ``A*exp(-0.5*((x-mu)/sigma)**2)``,
``table_support.independent`` --, the bound between them and ``SumModel.statement``, the rows that sit on the rules of
the statement, and the device entry point driven on padded rows.

The bound.  eps = 2**-53 is the relative error of one rounded operation; a faithful function (``pow10_dd``; numpy's
``exp``, ``log10`` and ``**`` are taken as faithful too) is off by at most 1 ulp <= 2 eps.  An error dq of an exponent
q enters 10**q as the relative error ln(10) |dq|.  To first order:

* POWERLAW, the statement.  lx = log10(x / x0): the quotient eps, which log10 turns into eps / ln(10) absolutely, and
  log10's own 2 eps |lx|.  G * lx: |G| times that and eps |G lx| of the product; logA - (.): eps |q|.  So
  |dq| <= eps (|G| / ln10 + 3 |G lx| + |q|), and with pow10_dd's 2 eps the value is off by
  eps (|G| + ln10 (3 |G lx| + |q|) + 2) relatively.  The independent form: 10**logA 2 eps, x / x0 eps, which ** -G
  turns into |G| eps, the power's own 2 eps, the product eps: (|G| + 5) eps.  Together
  R_pl = eps (2 |G| + ln10 (3 |G lx| + |q|) + 7).
* GAUSS, the statement.  d = (x - mu) / sigma: 2 eps.  q = (C d) d: d twice 4 eps, two products 2 eps, and C is the
  double nearest to -0.5 log10(e), eps: |dq| <= 7 eps |q|; pow10_dd 2 eps, times A eps: ln10 7 |q| eps + 3 eps.  The
  independent form: d 2 eps, its square 5 eps, the half exact, so the argument z = |q| ln10 of exp is off by 5 eps z;
  exp 2 eps, times A eps: 5 ln10 |q| eps + 3 eps.  Together R_g = eps (12 ln10 |q| + 6).
* TABLE: ``table_support.bound`` (absolute), derived there.
* the attenuation factor F = 10**(att N): q = att * N eps |q| on either side, the power 2 eps, the product with the sum
  eps: R_F = eps (2 ln10 |q| + 6).
* the adds: a sum of C values makes C roundings of partial sums that are at most sum |v_c| each, the last add a + u one
  more, on either side: 2 (C + 1) eps sum |v_c|.

|statement - independent| <= F (sum_att b_c) + sum_un b_c + (2 (C + 1) eps + R_F) F sum_att |v_c| + 2 (C + 1) eps
sum_un |v_c| with b_c = R |v_c| for the analytic components, taken 1.25 times for the terms of second order.  The
comparison is restricted to bins where every exponent has |q| <= 200: there the independent forms are accurate
themselves (beyond, exp and ** run into subnormal results).
"""
import numpy as np

from massivedatans_amd import _lib
from massivedatans_amd.summodel import GaussianLine, PowerLaw, SumModel
from massivedatans_amd.tablemodel import TableModel
import table_support
from table_support import EPS, make_model, random_params
from table_los_support import los_params, make_los_model, window_s

TILE = _lib.TABLE_TILE                                     # bins per workgroup of k_sum_curves
LN10 = float(np.log(10.0))
QMAX = 200.0


# ---- parameters ----
def component_params(c, x, rng, B, positive=False):
    """``B`` rows of component ``c``'s parameters on the abscissa ``x``."""
    if isinstance(c, TableModel):
        if c.extinction or c.broadening:
            return los_params(c, rng, B, window_s(c)[:3] if c.broadening else [0.0])
        return random_params(c, rng, B)
    if isinstance(c, PowerLaw):
        return np.column_stack((rng.uniform(-1.0, 1.0, size=B), rng.uniform(-1.0, 3.0, size=B)))
    span = max(float(x[-1] - x[0]), 1.0)
    A = 10 ** rng.uniform(-1, 1, size=B) * (1.0 if positive else rng.choice([-1.0, 1.0], size=B))
    return np.column_stack((A, rng.uniform(x[0] - 0.1 * span, x[-1] + 0.1 * span, size=B), span * 10 ** rng.uniform(-2.0, 0.0, size=B)))


def model_params(sm, x, rng, B, positive=False):
    cols = [component_params(c, x, rng, B, positive) for c in sm.components]
    if sm.att is not None:
        cols.append(rng.uniform(0.0, 2.0, size=(B, 1)))
    return np.ascontiguousarray(np.column_stack(cols))


def attenuation(x, seed=0):
    """A smooth negative exponent per unit N with a few positive bins: of either sign, as the statement allows."""
    rng = np.random.RandomState(seed)
    return -0.5 * (x[0] / x) ** 1.5 + 0.05 * rng.normal(size=len(x))


def rule_rows(sm, x, good):
    """Rows that the rules make NaN, and their names: from the good row ``good``, a NaN in every parameter in turn; +-inf
    in every parameter of an analytic component; sigma 0, -0.0 and negative; N +-inf."""
    rows, names = [], []

    def add(name, k, v):
        r = np.array(good, dtype=float)
        r[k] = v
        rows.append(r)
        names.append(name)
    for k in range(sm.ndim):
        add("NaN in parameter %d" % k, k, np.nan)
    for c, sl in zip(sm.components, sm.slices):
        if isinstance(c, TableModel):
            continue
        for k in range(sl.start, sl.stop):
            add("+inf in parameter %d" % k, k, np.inf)
            add("-inf in parameter %d" % k, k, -np.inf)
        if isinstance(c, GaussianLine):
            for v in (0.0, -0.0, -1.5):
                add("sigma = %r" % v, sl.start + 2, v)
    if sm.att is not None:
        add("N = +inf", sm.ndim - 1, np.inf)
        add("N = -inf", sm.ndim - 1, -np.inf)
    return np.ascontiguousarray(np.array(rows, dtype=float).reshape(-1, sm.ndim)), names


def edge_rows(sm, x, good):
    """Rows on the edges of the statement that are NOT NaN: sigma subnormal (d = +-inf, q = -299), G and logA that put q
    on and beyond the clamp, a line on a bin, N = 0 and N huge, A = 0 and negative."""
    rows, names = [], []

    def add(name, pairs):
        r = np.array(good, dtype=float)
        for k, v in pairs:
            r[k] = v
        rows.append(r)
        names.append(name)
    for c, sl in zip(sm.components, sm.slices):
        s = sl.start
        if isinstance(c, PowerLaw):
            for logA, G in ((299.0, 0.0), (300.0, 0.0), (-299.0, 0.0), (-1e308, 0.0), (0.0, 1e308), (0.0, -1e308), (1e308, 1e308)):
                add("power law logA=%g G=%g" % (logA, G), ((s, logA), (s + 1, G)))
        elif isinstance(c, GaussianLine):
            add("sigma subnormal", ((s + 2, 1e-320),))
            add("sigma huge", ((s + 2, 1e308),))
            add("mu on a bin", ((s + 1, x[len(x) // 2]),))
            add("mu huge", ((s + 1, -1e308),))
            add("A = 0", ((s, 0.0),))
            add("A = -0.0", ((s, -0.0),))
            add("A huge", ((s, -1e308),))
    if sm.att is not None:
        for N in (0.0, -0.0, 1e308, -1e308, 1e-320):
            add("N = %r" % N, ((sm.ndim - 1, N),))
    return np.ascontiguousarray(np.array(rows, dtype=float).reshape(-1, sm.ndim)), names


# ---- the independent forms and the bound ----
def independent_powerlaw(c, x, p):
    return 10 ** p[:, 0, None] * (x[None, :] / c.x0) ** -p[:, 1, None]


def independent_gauss(x, p):
    return p[:, 0, None] * np.exp(-0.5 * ((x[None, :] - p[:, 1, None]) / p[:, 2, None]) ** 2)


def independent(sm, x, xs):
    """``(value, bound, comparable)`` [B, nx] each: the sum made of the independent forms, the derived bound on its
    distance from the statement, and where every exponent has |q| <= QMAX."""
    xs = np.atleast_2d(np.asarray(xs, dtype=float))
    B, C = len(xs), len(sm.components)
    shape = (B, len(x))
    sums = {True: np.zeros(shape), False: np.zeros(shape)}          # the values, attenuated and not
    errs = {True: np.zeros(shape), False: np.zeros(shape)}          # the components' own bounds b_c
    mags = {True: np.zeros(shape), False: np.zeros(shape)}          # sum |v_c|
    ok = np.ones(shape, dtype=bool)
    for c, sl, attenuated in zip(sm.components, sm.slices, sm.attenuated):
        p = xs[:, sl]
        if isinstance(c, TableModel):
            v = table_support.independent(c, x, p)
            b = np.broadcast_to(table_support.bound(c, p), shape)
        elif isinstance(c, PowerLaw):
            v = independent_powerlaw(c, x, p)
            Glx = np.abs(p[:, 1, None] * np.log10(x / c.x0)[None, :])
            q = np.abs(p[:, 0, None] - p[:, 1, None] * np.log10(x / c.x0)[None, :])
            b = EPS * (2 * np.abs(p[:, 1, None]) + LN10 * (3 * Glx + q) + 7) * np.abs(v)
            ok &= q <= QMAX
        else:
            v = independent_gauss(x, p)
            q = 0.5 * np.log10(np.e) * ((x[None, :] - p[:, 1, None]) / p[:, 2, None]) ** 2
            b = EPS * (12 * LN10 * q + 6) * np.abs(v)
            ok &= q <= QMAX
        sums[attenuated] = sums[attenuated] + v
        errs[attenuated] = errs[attenuated] + b
        mags[attenuated] = mags[attenuated] + np.abs(v)
    F, RF = np.ones(shape), np.zeros(shape)
    if sm.att is not None:
        q = sm.att[None, :] * xs[:, -1, None]
        F = 10 ** q
        RF = EPS * (2 * LN10 * np.abs(q) + 6)
        ok &= np.abs(q) <= QMAX
    adds = 2 * (C + 1) * EPS
    value = sums[True] * F + sums[False]
    bound = 1.25 * (F * errs[True] + errs[False] + (adds + RF) * F * mags[True] + adds * mags[False])
    return value, bound, ok


# ---- the device entry point on padded rows ----
def dev_curves(lib, dsum, xs, pad=0, sentinel=-7.25):
    """``mdns_sum_curves_batch_dev`` on rows of nx + pad doubles pre-filled with ``sentinel``: the curves [B, nx] and
    whether the padding still holds the sentinel."""
    xs = np.ascontiguousarray(xs, dtype=float)
    B, nx = len(xs), dsum.nx
    ldc = nx + pad
    wide = np.full((B, ldc), sentinel)
    d_p, d_o = lib.mdns_dev_alloc(max(xs.nbytes, 8)), lib.mdns_dev_alloc(wide.nbytes)
    try:
        assert d_p and d_o
        _lib.check(lib.mdns_h2d(d_p, _lib.ptr(xs), xs.nbytes), "h2d")
        _lib.check(lib.mdns_h2d(d_o, _lib.ptr(wide), wide.nbytes), "h2d")
        _lib.check(lib.mdns_sum_curves_batch_dev(dsum.handle, d_p, B, d_o, ldc), "mdns_sum_curves_batch_dev")
        _lib.check(lib.mdns_sync(), "mdns_sync")
        _lib.check(lib.mdns_d2h(_lib.ptr(wide), d_o, wide.nbytes), "d2h")
    finally:
        for p in (d_p, d_o):
            if p:
                lib.mdns_dev_free(p)
    return np.ascontiguousarray(wide[:, :nx]), bool((wide[:, nx:] == sentinel).all())


# ---- models ----
def table(d, seed, nw=40, **kw):
    """A plain table (Part 12's first route) on the grid 300 .. 900."""
    return make_model(d, seed, nw=nw, **kw)


def los_table(d, seed, nw, **kw):
    """A table on the line-of-sight route with broadening (three kernels through S and R)."""
    return make_los_model(d, seed, nw=nw, **kw)


def positive_sum(x):
    """att x (power law + line) + a positive table the attenuation does not touch, all >= 0: what the draw tests and the
    whole runs fit.  Rows (logA, G, A, mu, sigma, p_0, p_1, z, At, N): 10 parameters."""
    from response_support import positive_model
    tm = positive_model()
    att = -0.3 * (x[0] / x) ** 2
    return SumModel([PowerLaw(x0=600.0), GaussianLine(), tm], attenuation=att, unattenuated=[2])


def positive_params(sm):
    """Rows of curves_support.gauss_prior, (A, mu, log10 sigma), as rows of ``positive_sum``: everything from mu and log
    sigma alone (the faint lines that filter_support._drive turns to stay draws from the whole prior)."""
    a0, a1 = sm.components[2].axes

    def convert(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        u1, u2 = (xs[:, 1] - 400.0) / 400.0, xs[:, 2] / 2.0
        u3, u4, u5, u6 = ((k * u1 + m * u2) % 1.0 for k, m in ((7.0, 3.0), (13.0, 5.0), (17.0, 11.0), (19.0, 23.0)))
        return np.ascontiguousarray(np.column_stack((
            -0.5 + u3, 3.0 * u4 - 1.0,                                   # logA, G
            0.2 + 2.0 * u5, 450.0 + 400.0 * u1, 5.0 + 40.0 * u2,          # A, mu, sigma
            a0[0] - 0.1 + (a0[-1] - a0[0] + 0.2) * u1, a1[0] - 0.1 + (a1[-1] - a1[0] + 0.2) * u2, 0.2 * u3, 0.5 * 10.0 ** u4,
            2.0 * u6)))                                                  # N
    return convert


def positive_prior(sm):
    """One parameter of ``positive_sum`` per dimension of the unit cube."""
    lo = np.array([-0.3, 0.0, 0.3, 500.0, 10.0, 0.0, -1.0, 0.0, 0.5, 0.0])
    hi = np.array([0.3, 2.0, 2.0, 800.0, 40.0, 1.6, 1.0, 0.2, 5.0, 1.5])
    assert len(lo) == sm.ndim
    return lambda us: lo + (hi - lo) * np.asarray(us, dtype=float)
