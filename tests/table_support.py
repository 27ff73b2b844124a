"""Test helper for the table model (tests/test_table_model_host.py, tests/test_table_model.py): tables with non-uniform
axes and grids, the INDEPENDENT form of the model -- ``A * numpy.interp(x / (1 + z), grid, multilinear template)`` with
the template made axis by axis --, the bound between it and ``TableModel.statement``, parameter sets that sit on every
edge of the statement, and the device entry points driven on padded rows.

The bound.  With eps = 2**-53 (the relative error of one rounded operation), Tm = max |T| over the table, f_a in [0, 1]
and all weights >= 0 (so sum_c |w_c| = sum_c w_c = 1 in exact arithmetic):

* a fraction f_a = (v - a_i) / (a_{i+1} - a_i) carries 3 eps (two differences, one quotient), 1 - f_a one more: every
  factor of a weight is off by at most 4 eps absolutely.  w_c is a product of d factors with d roundings of its own, so
  to first order  sum_c |dw_c| <= sum_a 4 eps * 2 + d eps = 9 d eps  (for a fixed axis a the products of the OTHER
  factors sum to 1 over each of the two knots of a);
* a corner value T0 + t (T1 - T0): |T1 - T0| <= 2 Tm; the difference 2 eps Tm, t's 3 eps on it 6 eps Tm, the product
  2 eps Tm, the sum 3 eps Tm: 13 eps Tm, and its size is at most Tm;
* the statement's sum over corners: sum_c |dw_c| Tm + 13 eps Tm + eps Tm (the products) + 2**d eps Tm (the additions,
  partial sums at most Tm): (9 d + 14 + 2**d) eps Tm;
* the independent form interpolates one axis at a time, V0 + f (V1 - V0), a convex step of the same 13 eps Tm per
  level, d levels, then numpy.interp's slope form along the grid, again at most 13 eps Tm: (13 d + 13) eps Tm.  This is
  the term for the different ORDER of the two interpolations: in exact arithmetic the two forms are the same
  polynomial in the f_a and t;
* both multiply by A once: eps |A| Tm each.

Both forms read the template at the same u = x / (1 + z) (the same two operations), so u itself adds nothing.  In all
|statement - independent| <= K(d) eps |A| Tm with K(d) = (9 d + 14 + 2**d) + (13 d + 13) + 2 = 22 d + 2**d + 29, taken
1.25 times for the terms of second order: 66.25 at d = 1, 166.25 at d = 4.
"""
import numpy as np

from massivedatans_amd import _lib
from massivedatans_amd.tablemodel import TableModel

EPS = 2.0 ** -53
TILE = _lib.TABLE_TILE                                     # channels per workgroup of k_table_curves


def bound_factor(d):
    return 1.25 * (22 * d + 2 ** d + 29)


def uneven(rng, n, lo, hi):
    """``n`` strictly increasing knots from ``lo`` to ``hi`` with steps that differ by up to a factor of 20."""
    steps = 10 ** rng.uniform(0, 1.3, size=n - 1)
    return lo + (hi - lo) * np.concatenate(([0.0], np.cumsum(steps) / steps.sum()))


def make_model(d, seed, lengths=None, nw=40, redshift=True, amplitude=True, grid_range=(300.0, 900.0)):
    """A table over ``d`` uneven axes (lengths 2, 5, 3, 4 unless given) and an uneven grid, values of either sign."""
    rng = np.random.RandomState(seed)
    lengths = list(lengths) if lengths is not None else [2, 5, 3, 4][:d]
    axes = [uneven(rng, n, -1.0 - a, 2.0 + 3 * a) for a, n in enumerate(lengths)]
    grid = uneven(rng, nw, *grid_range)
    smooth = np.sin(np.linspace(0, 9, nw))[None, :] * rng.uniform(0.5, 2, size=(int(np.prod(lengths)), 1))
    table = (smooth + 0.3 * rng.normal(size=smooth.shape)).reshape(lengths + [nw])
    return TableModel(axes, grid, table, redshift=redshift, amplitude=amplitude)


def abscissa(tm, nx, seed=0, beyond=0.1):
    """``nx`` ascending channels that reach ``beyond`` of the grid's length past both of its ends."""
    g0, g1 = tm.grid[0], tm.grid[-1]
    if nx == 1:
        return np.array([0.5 * (g0 + g1)])
    return np.sort(np.random.RandomState(seed).uniform(g0 - beyond * (g1 - g0), g1 + beyond * (g1 - g0), size=nx))


def random_params(tm, rng, B, beyond=0.15, zmax=0.5, decades=2.0):
    """Parameters of which a share lies outside every axis; z in [0, zmax], amplitudes over ``decades`` decades."""
    cols = [rng.uniform(a[0] - beyond * (a[-1] - a[0]), a[-1] + beyond * (a[-1] - a[0]), size=B) for a in tm.axes]
    if tm.redshift:
        cols.append(rng.uniform(0, zmax, size=B))
    if tm.amplitude:
        cols.append(10 ** rng.uniform(-decades / 2, decades / 2, size=B))
    return np.ascontiguousarray(np.column_stack(cols))


def edge_params(tm, x):
    """Rows and their names: every knot of every axis (first and last included), values below and above every axis,
    +-inf on every axis, z that puts u exactly on the first, a middle and the last grid knot for channel 0, z that puts
    every u below grid[0] / above grid[-1], z = -1, +-inf in z and A, negative and zero A; and, last, one row with a
    NaN in each parameter in turn."""
    mid = [0.5 * (a[0] + a[1]) for a in tm.axes]
    tail = ([0.25] if tm.redshift else []) + ([1.5] if tm.amplitude else [])
    rows, names = [], []

    def add(name, axis_values=None, z=None, A=None):
        r = list(axis_values if axis_values is not None else mid) + tail
        if z is not None and tm.redshift:
            r[tm.d] = z
        if A is not None and tm.amplitude:
            r[-1] = A
        rows.append(r)
        names.append(name)
    for a, axis in enumerate(tm.axes):
        for i, knot in enumerate(axis):
            add("axis %d knot %d" % (a, i), mid[:a] + [knot] + mid[a + 1:])
        for name, v in (("below", axis[0] - 1.0), ("above", axis[-1] + 1.0), ("-inf", -np.inf), ("+inf", np.inf),
                        ("just below", np.nextafter(axis[0], -np.inf)), ("just inside", np.nextafter(axis[-1], -np.inf))):
            add("axis %d %s" % (a, name), mid[:a] + [v] + mid[a + 1:])
    add("all first knots", [a[0] for a in tm.axes])
    add("all last knots", [a[-1] for a in tm.axes])
    if tm.redshift:
        for name, knot in (("first", tm.grid[0]), ("middle", tm.grid[len(tm.grid) // 2]), ("last", tm.grid[-1])):
            if x[0] != 0:
                add("u on the %s grid knot" % name, z=x[0] / knot - 1.0)
        big = max(abs(x).max(), 1.0)
        add("every u below the grid", z=4.0 * big / abs(tm.grid[0]) + 10.0)
        add("every u above the grid", z=-1.0 + 0.01 * abs(x[x != 0]).min() / abs(tm.grid[-1]) if (x != 0).any() else 0.0)
        add("z = 0", z=0.0)
        add("z = -1", z=-1.0)
        add("z = +inf", z=np.inf)
        add("z = -inf", z=-np.inf)
    if tm.amplitude:
        for A in (0.0, -2.0, np.inf, -np.inf, 1e-300, 1e300):
            add("A = %g" % A, A=A)
    first_nan = len(rows)
    for k in range(tm.ndim):
        r = list(mid) + tail
        r[k] = np.nan
        rows.append(r)
        names.append("NaN in parameter %d" % k)
    return np.ascontiguousarray(np.array(rows, dtype=float)), names, first_nan


def independent(tm, x, xs):
    """``A * numpy.interp(x / (1 + z), grid, template)`` per candidate, the template interpolated one axis after the
    other (last axis first) with fractions from numpy.interp on the knot numbers: another order of the same
    polynomial, none of the statement's code."""
    xs = np.atleast_2d(np.asarray(xs, dtype=float))
    out = np.empty((len(xs), len(x)))
    for b, row in enumerate(xs):
        V = tm.table
        for a in reversed(range(tm.d)):
            axis = tm.axes[a]
            pos = np.interp(row[a], axis, np.arange(len(axis), dtype=float))        # knot number, clamped at the ends
            i = min(int(np.floor(pos)), len(axis) - 2)
            f = (min(max(row[a], axis[0]), axis[-1]) - axis[i]) / (axis[i + 1] - axis[i])
            V0, V1 = np.take(V, i, axis=a), np.take(V, i + 1, axis=a)
            V = V0 + f * (V1 - V0)
        u = x / (1.0 + row[tm.d]) if tm.redshift else x
        out[b] = np.interp(u, tm.grid, V)
        if tm.amplitude:
            out[b] = row[-1] * out[b]
    return out


def bound(tm, xs):
    """[B, 1]: the derived bound on |statement - independent| per candidate (module docstring)."""
    A = np.abs(np.atleast_2d(xs)[:, -1]) if tm.amplitude else np.ones(len(np.atleast_2d(xs)))
    return (bound_factor(tm.d) * EPS * np.abs(tm.table).max() * A)[:, None]


def same_bits(a, b):
    """Equal bit for bit where both are numbers, NaN in the same places (a NaN's payload is not part of the statement)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def dev_curves(lib, table, xs, pad=0, sentinel=-7.25):
    """``mdns_table_curves_batch_dev`` on rows of nx + pad doubles pre-filled with ``sentinel``: the curves [B, nx] and
    whether the padding still holds the sentinel."""
    xs = np.ascontiguousarray(xs, dtype=float)
    B, nx = len(xs), table.nx
    ldc = nx + pad
    wide = np.full((B, ldc), sentinel)
    d_p, d_o = lib.mdns_dev_alloc(max(xs.nbytes, 8)), lib.mdns_dev_alloc(wide.nbytes)
    try:
        assert d_p and d_o
        _lib.check(lib.mdns_h2d(d_p, _lib.ptr(xs), xs.nbytes), "h2d")
        _lib.check(lib.mdns_h2d(d_o, _lib.ptr(wide), wide.nbytes), "h2d")
        _lib.check(lib.mdns_table_curves_batch_dev(table.handle, d_p, B, d_o, ldc), "mdns_table_curves_batch_dev")
        _lib.check(lib.mdns_sync(), "mdns_sync")
        _lib.check(lib.mdns_d2h(_lib.ptr(wide), d_o, wide.nbytes), "d2h")
    finally:
        for p in (d_p, d_o):
            if p:
                lib.mdns_dev_free(p)
    return np.ascontiguousarray(wide[:, :nx]), bool((wide[:, nx:] == sentinel).all())


def posterior_moments(results):
    """Posterior mean and standard deviation [ndata, ndim] of a finished run from ``results['weights']``."""
    _, x, L, w, _ = list(zip(*results["weights"]))
    x, lw = np.array(x), np.array(w) + np.array(L)
    lw = np.where(np.isfinite(lw), lw, -np.inf)
    p = np.exp(lw - lw.max(axis=0))
    p /= p.sum(axis=0)
    mean = (p[:, :, None] * x).sum(axis=0)
    std = np.sqrt((p[:, :, None] * (x - mean[None]) ** 2).sum(axis=0))
    return mean, std
