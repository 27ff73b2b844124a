"""Test helper for the table model's line-of-sight effects (tests/test_table_los_host.py, tests/test_table_los.py):
models with an extinction curve and a broadening on the uneven tables of ``table_support``, parameter sets whose ``s``
takes the window sizes that matter, the two INDEPENDENT forms, and the bounds between them and
``TableModel.statement``.

Both bounds are derived here from the operations of the two forms, not from what they are seen to differ by.  eps =
2**-53 is the relative error of one rounded operation, Tm = max |T| over the table, weights w_c >= 0 with sum 1 in exact
arithmetic.  ``table_support`` shows sum_c |dw_c| <= 9 d eps, that a linear step V0 + f (V1 - V0) or numpy.interp's
slope form on values of size <= V is off by <= 13 eps V, and that the axis-by-axis template is off by <= 13 d eps Tm.

The bound with extinction (no broadening).  Q = max_m |ext[m] E| (at most 299), P = max_m 10 ** (ext[m] E).

* statement: the blend S_m = sum_c w_c T_c[m]: 9 d eps Tm (weights) + eps Tm (products) + 2**d eps Tm (additions, partial
  sums <= Tm).  q = ext[m] * E is one rounding, eps |q| on the exponent, a factor 1 + ln(10) Q eps on 10 ** q; pow10_dd
  is one faithful rounding (less than one ulp: 2 eps); the product one more.  So S_m P_m is off by
  (9 d + 2**d + 4 + ln(10) Q) eps Tm P, and the step along the grid adds 13 eps Tm P:
  (9 d + 2**d + 17 + ln(10) Q) eps Tm P;
* independent: the template 13 d eps Tm; ext * E the same rounding, ln(10) Q eps; ``10.0 ** v`` is the C library's pow
  or numpy's own loop: the C library documents 1 ulp, numpy's accuracy tests hold its loops to 4 ulp -- the larger,
  8 eps; the product eps; numpy.interp 13 eps Tm P: (13 d + 22 + ln(10) Q) eps Tm P;
* both multiply by A: eps each.

|statement - independent| <= KE eps |A| Tm P with KE = 22 d + 2**d + 41 + 2 ln(10) Q, taken 1.25 times for the terms of
second order.

The bound with broadening (no extinction), every table value > 0, s > 0, L the longest window in knots.  A weighted
mean with positive weights of values of size <= Tm moves by <= e Tm when every weight moves by a relative e, and by as
much as its values move.

* statement: S_m off by (9 d + 1 + 2**d) eps Tm (above).  d_mn: three roundings (difference, two quotients), 3 eps
  relative; (C d) d two more: the exponent a = C d^2 carries 8 eps relative, |a| ln(10) = d^2 / 2 <= 12.5: a factor
  1 + 100 eps on 10 ** a; pow10_dd 2 eps; times the width eps (the widths are the same numbers in both forms): every K_n
  is off by 103 eps relative, in num and in den: 206 eps Tm.  The products S_n K_n eps; the two sums of L positive terms
  (L - 1) eps each; the quotient eps: (9 d + 2**d + 209 + 2 L) eps Tm;
* independent: the template 13 d eps Tm.  delta = g_n / g_m - 1 CANCELS: the quotient's rounding, eps (1 + |delta|), stays
  absolute, and the difference adds eps |delta|; / s is one more rounding: d is off by eps (1 + 2 |delta|) / |delta| + eps
  relative.  The exponent d^2 / 2 (square one rounding, taken as 2) is off by d^2 (e_d + eps) absolutely, at most
  |d| (1 + 2 |delta|) eps / s + 2 d^2 eps <= (5 (1 + 10 s) / s + 50) eps <= (5 / s + 100) eps for |d| <= 5.  numpy.exp: 8
  eps, as for pow; the width eps: 5 / s + 109 eps relative per weight, in the product and in the row sum:
  (10 / s + 218) eps Tm.  ``@`` adds, in whatever order, L - 1 times two numbers that are not zero, with a rounding of
  every product; the row sum L - 1 likewise; the normalisation eps: (2 L + 2) eps Tm more:
  (13 d + 10 / s + 220 + 2 L) eps Tm;
* the step along the grid, 13 eps Tm in each form, and A, eps in each: 28 eps Tm.

|statement - independent| <= KB eps |A| Tm with KB = 22 d + 2**d + 457 + 10 / s + 4 L, taken 1.25 times.  The two forms
must agree on who is in a window: a term at the cut is worth e**-12.5, far above the bound, so the test asserts that no
|d_mn| lies within 1e-9 of the cut (the two forms' d differ by far less: e_d |d| <= 1e-12 for s >= 1e-3).
"""
import numpy as np

from massivedatans_amd import _lib
from massivedatans_amd.tablemodel import BROADEN_CUT, TableModel
from table_support import EPS, independent, make_model, uneven  # noqa: F401  (re-exported)

TILE = _lib.TABLE_TILE                                     # template knots per workgroup of k_table_los_blend / _broaden


def make_los_model(d, seed, lengths=None, nw=40, redshift=True, amplitude=True, extinction=True, broadening=True, positive=False):
    """``table_support.make_model``'s table (uneven axes and grid on [300, 900], values of either sign unless
    ``positive``: then in [1, 3]) with an extinction curve of either sign, steeper towards the blue, and the broadening."""
    base = make_model(d, seed, lengths=lengths, nw=nw, redshift=redshift, amplitude=amplitude)
    rng = np.random.RandomState(seed + 1000)
    table = 1.0 + 2.0 * rng.uniform(size=base.table.shape) if positive else base.table
    ext = -0.4 * (3.1 * (base.grid[0] / base.grid) ** 1.3 - 0.8 + 0.05 * rng.normal(size=nw)) if extinction else None
    return TableModel(base.axes, base.grid, table, redshift=redshift, amplitude=amplitude, extinction=ext, broadening=broadening)


def plain_of(tm):
    """The same table with neither effect, no z and no A: what ``table_support.independent`` blends templates of."""
    return TableModel(tm.axes, tm.grid, tm.table)


def window_s(tm):
    """Four values of s by the windows they give on ``tm.grid``: 0, one whose every window is {m}, one of about +-7
    knots, one that covers the whole grid from every knot."""
    g = tm.grid
    only_m = float((np.diff(g) / g[1:]).min()) / (2.0 * BROADEN_CUT)
    seven = 7.0 * float(np.mean(np.diff(g) / g[1:])) / BROADEN_CUT
    whole = 1.5 * float((g[-1] - g[0]) / g[0]) / BROADEN_CUT
    return [0.0, only_m, seven, whole]


def los_params(tm, rng, B, s_values, beyond=0.15, zmax=0.5, emax=1.0, decades=2.0):
    """``B`` rows (p .. [, z] [, E] [, s] [, A]): a share of the p outside every axis, E of both signs in [-emax, emax],
    s going round ``s_values``."""
    cols = [rng.uniform(a[0] - beyond * (a[-1] - a[0]), a[-1] + beyond * (a[-1] - a[0]), size=B) for a in tm.axes]
    if tm.redshift:
        cols.append(rng.uniform(0, zmax, size=B))
    if tm.extinction:
        cols.append(rng.uniform(-emax, emax, size=B))
    if tm.broadening:
        cols.append(np.array([s_values[b % len(s_values)] for b in range(B)]))
    if tm.amplitude:
        cols.append(10 ** rng.uniform(-decades / 2, decades / 2, size=B))
    return np.ascontiguousarray(np.column_stack(cols))


def special_rows(tm, x):
    """Rows and their names, and the index of the first row that must be NaN: E that puts q on and beyond +-299,
    windows of every size, u on the first, a middle and the last knot; then E = +-inf, s < 0, s = +-inf and a NaN in
    each parameter in turn."""
    mid = [0.5 * (a[0] + a[1]) for a in tm.axes]
    s_all = window_s(tm)
    base = list(mid) + ([0.25] if tm.redshift else []) + ([0.3] if tm.extinction else []) + ([s_all[2]] if tm.broadening else []) + \
        ([1.5] if tm.amplitude else [])
    rows, names = [], []

    def add(name, **kw):
        r = list(base)
        for key, v in kw.items():
            at = {"z": tm.d, "E": tm.at_e, "s": tm.at_s}[key]
            r[at] = v
        rows.append(r)
        names.append(name)
    add("plain")
    if tm.extinction:
        # (where ext holds +-1.0 exactly, as the edge tests make it, E = +-299 puts q exactly on the clamp)
        for E in (299.0, -299.0, 400.0, -400.0, 0.0, -0.0, 1e300, -1e300):
            add("E = %r" % E, E=E)
    if tm.broadening:
        for name, s in zip(("s = 0", "windows {m}", "+-7 knots", "whole grid"), s_all):
            add(name, s=s)
        add("s = -0.0", s=-0.0)                                            # (>= 0 and not > 0: R = S, a number)
        add("s tiny", s=1e-300)
    if tm.redshift and x[0] != 0:
        for name, knot in (("first", tm.grid[0]), ("middle", tm.grid[len(tm.grid) // 2]), ("last", tm.grid[-1])):
            add("u on the %s knot" % name, z=x[0] / knot - 1.0)
    first_nan = len(rows)
    if tm.extinction:
        add("E = +inf", E=np.inf)
        add("E = -inf", E=-np.inf)
    if tm.broadening:
        add("s < 0", s=-1e-3)
        add("s = +inf", s=np.inf)
        add("s = -inf", s=-np.inf)
    for k in range(tm.ndim):
        r = list(base)
        r[k] = np.nan
        rows.append(r)
        names.append("NaN in parameter %d" % k)
    return np.ascontiguousarray(np.array(rows, dtype=float)), names, first_nan


# ---- the independent forms and their bounds (module docstring) ----
def independent_extinction(tm, x, xs):
    """``A * numpy.interp(x / (1 + z), grid, template * 10.0 ** (ext * E))``, the template blended axis by axis."""
    xs = np.atleast_2d(np.asarray(xs, dtype=float))
    templates = independent(plain_of(tm), tm.grid, xs[:, :tm.d])           # read at the knots themselves
    out = np.empty((len(xs), len(x)))
    for b, row in enumerate(xs):
        u = x / (1.0 + row[tm.d]) if tm.redshift else x
        out[b] = np.interp(u, tm.grid, templates[b] * 10.0 ** (tm.ext * row[tm.at_e]))
        if tm.amplitude:
            out[b] = row[-1] * out[b]
    return out


def bound_extinction(tm, xs):
    xs = np.atleast_2d(xs)
    A = np.abs(xs[:, -1]) if tm.amplitude else np.ones(len(xs))
    q = np.abs(tm.ext[None, :] * xs[:, tm.at_e, None])
    K = 22 * tm.d + 2 ** tm.d + 41 + 2 * np.log(10.0) * q.max(axis=1)
    return (1.25 * K * EPS * A * np.abs(tm.table).max() * 10.0 ** q.max(axis=1))[:, None]


def dense_d(tm, s):
    """d_mn [nw, nw] in the independent form's arithmetic."""
    g = tm.grid
    return (g[None, :] / g[:, None] - 1.0) / s


def independent_broadening(tm, x, xs):
    """A dense row-normalised [nw, nw] matrix of ``exp(-0.5 ((g_n / g_m - 1) / s)^2) * width_n`` inside the cut, applied
    with ``@`` to the axis-by-axis template, then ``A * numpy.interp``."""
    xs = np.atleast_2d(np.asarray(xs, dtype=float))
    templates = independent(plain_of(tm), tm.grid, xs[:, :tm.d])
    out = np.empty((len(xs), len(x)))
    for b, row in enumerate(xs):
        dmn = dense_d(tm, row[tm.at_s])
        M = np.where(np.abs(dmn) <= BROADEN_CUT, np.exp(-0.5 * dmn ** 2) * tm.delta[None, :], 0.0)
        M = M / M.sum(axis=1)[:, None]
        u = x / (1.0 + row[tm.d]) if tm.redshift else x
        out[b] = np.interp(u, tm.grid, M @ templates[b])
        if tm.amplitude:
            out[b] = row[-1] * out[b]
    return out


def longest_window(tm, s):
    return int((np.abs(dense_d(tm, s)) <= BROADEN_CUT).sum(axis=1).max())


def bound_broadening(tm, xs):
    xs = np.atleast_2d(xs)
    A = np.abs(xs[:, -1]) if tm.amplitude else np.ones(len(xs))
    s = xs[:, tm.at_s]
    L = np.array([longest_window(tm, v) for v in s])
    K = 22 * tm.d + 2 ** tm.d + 457 + 10.0 / s + 4 * L
    return (1.25 * K * EPS * A * np.abs(tm.table).max())[:, None]
