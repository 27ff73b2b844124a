"""Test helper for the W statistic of count spectra with a background (tests/test_wstat_curves_host.py,
tests/test_wstat_curves.py): low-count source and background spectra with exposures and bad pixels, the numpy statement
of the likelihood, the float64 emulation of the kernel's chain, and the bound between the two.

The statement (include/mdns.h Part 11), with tiny = DBL_MIN and c' = c for c >= 0, NaN otherwise; per pixel n, e
(source region: counts, exposure) and b, g (background region), T = e + g, N = n + b, a = N - T c':

    d = sqrt(a^2 + 4 T b c');   f = (a + d) / (2 T) for a >= 0,   f = 2 b c' / (d - a) for a < 0;   s = c' + f
    L = sum_j ( n log(max(s, tiny)) + b log(max(f, tiny)) - e s - g f ) + Kw
    Kw = sum over n > 0 of n (1 + log e - log n) + sum over b > 0 of b (1 + log g - log b)

f maximises the bracket over f >= 0: it is the root of T f^2 - a f - b c' = 0, and BOTH forms give it for every a; the
branch only avoids the cancellation.  A masked pixel (T = 0) has f = 0.

The chain (csrc/mdns_curves.hip, k_curve_rows_b), every operation one rounded float64 one, per pixel

    T = e + g;  N = n + b;  Q = 4 (T b);  T2 = 2 T (1 where T == 0);  b2 = 2 b

and per (curve, spectrum) pair, channels ascending, acc = +0:

    a = fma(-T, c', N);  d = sqrt(fma(a, a, Q c'));  f = (a + d) / T2 if a >= 0 else (b2 c') / (d - a);  s = c' + f
    acc = fma(n, log(fmax(s, tiny)), acc);  acc = fma(b, log(fmax(f, tiny)), acc);  acc = fma(-e, s, acc);
    acc = fma(-g, f, acc);                                                        L = acc + Kw (the statement's, rounded)

The bound.  u = 2**-53; +, *, fma round once, |delta| <= u.  sqrt and / err by at most r = SQRT_DIV_ULPS 2**-52
relatively, the logarithm by lam = LOG_ULPS 2**-52.  Written for the exact T, N ... of the uploaded float64 values; to
first order in u unless said, and what is second order lives in the slack named at the end.

(1) The error of f.  With A = N + T c' (>= |a|, and >= d, since d^2 = a^2 + 4 T b c' <= a^2 + 4 (T c') N <= A^2):
    |a^ - a| <= u N + u T c' + u |a| <= 2 u A                       (T^ and N^ carry one rounding each, the fma one)
    r = d^2:  |r^ - r| <= 2 |a| 2 u A + 3 u (4 T b c') + u r <= 4 u A d + 4 u d^2      (Q^ c' carries three roundings)
    |sqrt(r^) - d| = |r^ - r| / (sqrt(r^) + d) <= 4 u A + 4 u d, so |d^ - d| <= (8 u + r) A     (no expansion needed)
  upper branch, f = (a + d) / (2 T):  |num^ - num| <= 2 u A + (8 u + r) A + u (a + d) <= (12 u + r) A, and the division
    by 2 T^ adds (u + r) f:  |f^ - f| <= (6 u + r / 2)(c' + N / T) + (u + r) f
  lower branch, f = 2 b c' / (d - a):  the numerator errs by u, the denominator by (8 u + r) A + 2 u A + u (d + |a|)
    <= (12 u + r) A, i.e. relatively by (12 u + r) A / (d - a); f A / (d - a) = 2 b c' A / (d - a)^2 <= A / (2 T)
    because (d - a)^2 >= d^2 >= 4 T b c' for a <= 0: again |f^ - f| <= (6 u + r / 2)(c' + N / T) + (u + r) f
  Both forms are the same number, so a computed a^ of the other sign than a (|a| <= 2 u A then) changes nothing in the
  argument, except that (d - a)^2 >= 4 T b c' needs a <= 0: there 2 a d <= 4 u A d is second order against d^2 unless
  d itself is O(u A), where f = O(u A / T) is below the bound altogether.  With G = c' + f + N / T and r = 2 u (one
  ulp, twice the correct rounding assumed below) the larger coefficient is 7 u:

    |f^ - f| <= FU u G,   FU = 8         (7, and one for the second-order terms)

(2) What it does to a term.  s^ = (c' + f^)(1 + delta): |s^ - s| <= |f^ - f| + u s.  The logarithms are Lipschitz 1/s
and 1/f (the clamp at tiny only flattens them), so the four summands move by at most
    n (lam |l1| + u + |f^ - f| / s) + b (lam |l2| + |f^ - f| / f) + e (|f^ - f| + u s) + g |f^ - f|
  = lam (n |l1| + b |l2|) + u (n + e s) + |f^ - f| (n / s + b / f + T).
f is the stationary point, n / s + b / f = T where f > 0; where f = 0 (b = 0, a <= 0) n / s <= T and b / f drops out
with b.  Either way N <= T s, so n <= T s and G T = T s + N <= 2 T s:
    |f^ - f| (n / s + b / f + T) <= 2 T FU u G <= 4 FU u T s.
(The first-order effect of f's error on the term CANCELS at the stationary point -- that is why the measured errors sit
far below this; the bound takes absolute values and does not use it.)

(3) The chain: the products inside the fmas are exact, 4 nx terms enter a running sum that rounds once per fma, and
the last addition of Kw^ = Kw (1 + delta) rounds once more: at most 4 nx + 1 factors behind any term,
    ((1 + u)^(4 nx + 1) - 1)(sum |t_i| + |Kw|) <= (4 nx + 2) u S,    S = sum_j (n |l1| + b |l2| + e s + g f) + |Kw|.

Together, with F = sum_j T s (>= sum_j e s and >= sum_j n), and two steps of slack in the first coefficient for the cross
terms and for the longdouble statement's own error (2**-11 of the bound's), as tests/poisson_support.py takes them:

    bound = (4 nx + 5) u S  +  LOG_ULPS 2**-52 sum_j (n |l1| + b |l2|)  +  (4 FU + 1) u F

LOG_ULPS: HIP's table of math-function accuracy gives 1 ulp for the fp64 ``log`` (tests/poisson_support.py: an
assumption, no copy ships with the toolkit; the tests take twice that).  SQRT_DIV: the toolkit ships no statement on
its fp64 ``sqrt`` and ``/`` either.  Without fast-math the compiler lowers ``/`` to the scale / fmas / fixup sequence
and ``sqrt`` to a refined reciprocal square root, both meant to round correctly (half an ulp): an ASSUMPTION as well,
and the tests take twice that, one ulp.  tests/test_wstat_curves.py measures the device's f against the exactly
emulated one."""
import numpy as np

from massivedatans_amd.like import background_pixels
from poisson_support import LOG_ULPS, TINY, U, _fma, count_data

SQRT_DIV_ULPS_ASSUMED = 0.5                          # correctly rounded
SQRT_DIV_ULPS = 2 * SQRT_DIV_ULPS_ASSUMED
FU = 8                                               # |f^ - f| <= FU u (c' + f + N / T)  (module docstring, (1))
LD = np.longdouble


def bound(nx, S, logs, F):
    """|L - L_statement| <= bound (module docstring): ``S`` = sum (n |l1| + b |l2| + e s + g f) + |Kw|, ``logs`` = sum
    (n |l1| + b |l2|), ``F`` = sum (e + g)(c' + f)."""
    return (4 * nx + 5) * U * S + LOG_ULPS * 2.0 ** -52 * logs + (4 * FU + 1) * U * F


def rate_bound(c, f, N, T):
    """|f - f_statement| <= this, where T > 0 (module docstring, (1))."""
    return FU * U * (c + f + N / T)


def wstat_data(ndata, nx, seed=0, exposure=True, edges=True):
    """poisson_support.count_data's spectra (levels 0.05 to 50 counts per pixel, e in [0.5, 2] with 5 % zeros, 1 % NaN
    counts, an all-zero and a fully masked spectrum) read as SOURCE rates, plus per spectrum a background of its own
    level between 0.05 and 50 counts per pixel (log-uniform), seen in the source region (added to ``y``) and in a
    background region with exposures g uniform in [0.5, 8] (the area ratio), 5 % of them planted 0, and 1 % of the
    background counts NaN.  ``exposure=False``: neither e nor g is given (ones).  ``edges``: the all-zero spectrum has no
    background counts either.  Returns dict(x, y, e, b, g), the four of shape [nx, ndata]."""
    d = count_data(ndata, nx, seed=seed, exposure=exposure, edges=edges)
    rng = np.random.RandomState([seed, ndata, nx, 7])
    level = 10 ** rng.uniform(np.log10(0.05), np.log10(50.0), size=ndata)
    g = rng.uniform(0.5, 8.0, size=d["y"].shape)
    g[rng.uniform(size=g.shape) < 0.05] = 0.0
    e = d["e"] if exposure else np.ones_like(g)
    if not exposure:
        g = np.ones_like(g)
    with np.errstate(invalid="ignore"):
        y = d["y"] + rng.poisson(level[None, :] * e)
    b = rng.poisson(level[None, :] * g).astype(float)
    b[rng.uniform(size=g.shape) < 0.01] = np.nan
    if not exposure:
        b[rng.uniform(size=g.shape) < 0.05] = np.inf              # (what masks a pixel when no g can)
    if edges and ndata >= 3:
        y[:, ndata // 3] = 0.0
        b[:, ndata // 3] = 0.0
    return dict(x=d["x"], y=y, e=d["e"], b=b, g=g if exposure else None)


def _rate(c, n, e, b, g, dtype):
    """The statement's f for broadcastable arrays (c: c', NaN where invalid): 0 where T = 0."""
    c, n, e, b, g = (np.asarray(a).astype(dtype) for a in (c, n, e, b, g))
    T, N = e + g, n + b
    a = N - T * c
    d = np.sqrt(a * a + 4 * T * b * c)
    with np.errstate(invalid="ignore", divide="ignore"):
        up = (a + d) / np.where(T == 0, dtype(1), 2 * T)
        down = 2 * b * c / np.where(a < 0, d - a, dtype(1))
    return np.where(a >= 0, up, np.where(a < 0, down, dtype(np.nan)))


class NumpyWstat(object):
    """``loglike_batch(curves[B, nx], mask)``: the statement over source counts ``y`` and exposures ``e``, background
    counts ``b`` and exposures ``g`` (None: ones) of shape [nx, ndata], with the masking rule and the float64 offsets of
    like.background_pixels.  ``loglike_batch_long``: the same in np.longdouble with the offsets not rounded.
    ``background_fit[_long]``: f [B, M, nx].  ``sums_long``: (S, logs, F) of every pair, for ``bound``."""

    def __init__(self, y, e=None, b=None, g=None):
        self.y, self.e, self.b, self.g, self.masked, self.Kw = background_pixels(y, e, b, g)
        self.ndata = self.y.shape[1]
        self.n_masked = self.masked.sum(axis=0)
        self.Kw_long = LD(0)
        for n, ee in ((self.y, self.e), (self.b, self.g)):
            good = n > 0
            nn, el = np.where(good, n, 1.0).astype(LD), np.where(good, ee, 1.0).astype(LD)
            self.Kw_long = self.Kw_long + np.where(good, nn * (1 + np.log(el) - np.log(nn)), LD(0)).sum(axis=0)
        assert np.array_equal(self.Kw_long.astype(np.float64), self.Kw)

    def _parts(self, curves, data_mask, dtype):
        """Per pair and channel, [B, nx, M]: c', f, s, l1, l2 and the data [nx, M]."""
        c = np.atleast_2d(np.asarray(curves, dtype=float))
        c = np.where(c >= 0, c, np.nan).astype(dtype)[:, :, None]
        sel = slice(None) if data_mask is None else np.asarray(data_mask)
        n, e, b, g = (a[:, sel].astype(dtype) for a in (self.y, self.e, self.b, self.g))
        with np.errstate(invalid="ignore"):
            f = _rate(c, n[None], e[None], b[None], g[None], dtype)
            s = c + f
            l1, l2 = np.log(np.fmax(s, dtype(TINY))), np.log(np.fmax(f, dtype(TINY)))
        Kw = (self.Kw if dtype is np.float64 else self.Kw_long)[sel]
        return c, f, s, l1, l2, n, e, b, g, Kw

    def _sum(self, curves, data_mask, dtype):
        c, f, s, l1, l2, n, e, b, g, Kw = self._parts(curves, data_mask, dtype)
        with np.errstate(invalid="ignore"):
            return (n * l1 + b * l2 - e * s - g * f).sum(axis=1) + Kw

    def loglike_batch(self, curves, data_mask=None):
        return self._sum(curves, data_mask, np.float64)

    def loglike_batch_long(self, curves, data_mask=None):
        return self._sum(curves, data_mask, LD)

    def background_fit(self, curves, data_mask=None, dtype=np.float64):
        return np.ascontiguousarray(np.swapaxes(self._parts(curves, data_mask, dtype)[1], 1, 2))

    def background_fit_long(self, curves, data_mask=None):
        return self.background_fit(curves, data_mask, LD)

    def sums_long(self, curves, data_mask=None):
        c, f, s, l1, l2, n, e, b, g, Kw = self._parts(curves, data_mask, LD)
        with np.errstate(invalid="ignore"):
            logs = (n * np.abs(l1) + b * np.abs(l2)).sum(axis=1)
            S = logs + (e * s + g * f).sum(axis=1) + np.abs(Kw)
            F = ((e + g) * s).sum(axis=1)
        return S, logs, F

    def branches(self, curves, data_mask=None):
        """Over the unmasked pixels of every pair: (share with a >= 0, share with a < 0, number with |a| <= 1e-3 A)."""
        c = np.atleast_2d(np.asarray(curves, dtype=float))[:, :, None]
        sel = slice(None) if data_mask is None else np.asarray(data_mask)
        n, e, b, g = (a[None, :, sel] for a in (self.y, self.e, self.b, self.g))
        T, N = e + g, n + b
        a, A = N - T * c, N + T * c
        live = np.broadcast_to(T > 0, a.shape)
        return float((a >= 0)[live].mean()), float((a < 0)[live].mean()), int((np.abs(a) <= 1e-3 * A)[live & (A > 0)].sum())


def within_bound(got, statement, nx, curves, data_mask=None, whole=None):
    """``(ok, worst)``: whether every ``got`` [B, M] lies within ``bound`` of ``statement.loglike_batch_long`` (a NaN
    exactly where the statement has one), and the largest error in units of the bound.  ``whole``: (statement, S, logs,
    F) over ALL spectra, computed once by the caller; the selection's columns are taken from it."""
    if whole is None:
        whole, data_mask = (statement.loglike_batch_long(curves, data_mask),) + statement.sums_long(curves, data_mask), None
    want, S, logs, F = (a if data_mask is None else a[:, np.asarray(data_mask)] for a in whole)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    lim = bound(nx, *(a[~nan].astype(float) for a in (S, logs, F)))
    err = np.abs(got[~nan].astype(LD) - want[~nan]).astype(float)
    zero = lim == 0
    if (err[zero] != 0).any():
        return False, np.inf
    worst = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    return worst <= 1.0, worst


def rate_within_bound(got, statement, curves, data_mask=None):
    """``(ok, worst)`` for ``got`` = f [B, M, nx] against the longdouble f: within ``rate_bound`` where T > 0, exactly 0
    at a masked pixel, NaN exactly along an invalid curve value."""
    want = statement.background_fit_long(curves, data_mask)
    sel = slice(None) if data_mask is None else np.asarray(data_mask)
    n, e, b, g = (a[:, sel].T[None].astype(LD) for a in (statement.y, statement.e, statement.b, statement.g))
    T, N = np.broadcast_to(e + g, want.shape), np.broadcast_to(n + b, want.shape)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    dead = (T == 0) & ~nan
    if (got[dead] != 0).any() or (want[dead] != 0).any():
        return False, np.inf
    live = (T > 0) & ~nan
    c = np.broadcast_to(np.atleast_2d(np.asarray(curves, dtype=float))[:, None, :], want.shape)[live].astype(LD)
    lim = rate_bound(c, want[live], N[live], T[live]).astype(float)
    err = np.abs(got[live].astype(LD) - want[live]).astype(float)
    zero = lim == 0
    if (err[zero] != 0).any():
        return False, np.inf
    worst = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    return worst <= 1.0, worst


def _sqrt(x):
    """The correctly rounded square root of a float64 x >= 0: numpy's (IEEE requires it of the hardware instruction)."""
    return float(np.sqrt(np.float64(x)))


def rate(c, n, e, b, g):
    """The kernel's f for one pixel in float64, operation by operation (sqrt and / correctly rounded)."""
    if not c >= 0:
        return float("nan")
    T, N = e + g, n + b
    Q = 4.0 * (T * b)
    T2 = 1.0 if T == 0.0 else 2.0 * T
    a = _fma(-T, c, N)
    d = _sqrt(_fma(a, a, Q * c))
    if a >= 0.0:
        return (a + d) / T2
    return (2.0 * b * c) / (d - a)


def chain(c, n, e, b, g, Kw, log=None):
    """The kernel's chain for one pair in float64, operation by operation: curve ``c``, the four data columns f64[nx] as
    uploaded (background_pixels), offset ``Kw``.  ``log``: the logarithm to use (default numpy's)."""
    log = (lambda v: float(np.log(np.float64(v)))) if log is None else log
    acc = 0.0
    for cc, nn, ee, bb, gg in zip(*(np.asarray(a, dtype=float).tolist() for a in (c, n, e, b, g))):
        cp = cc if cc >= 0 else float("nan")
        f = rate(cp, nn, ee, bb, gg)
        s = cp + f
        acc = _fma(nn, log(s if s >= TINY else TINY), acc)          # (fmax drops a NaN: log(tiny))
        acc = _fma(bb, log(f if f >= TINY else TINY), acc)
        acc = _fma(-ee, s, acc)
        acc = _fma(-gg, f, acc)
    return acc + float(Kw)


def source_model(x, gain=40.0, floor=0.0):
    """``model(xs[B, 3]) -> curves[B, nx]``, source count rates >= 0 for rows (A, mu, log10 sig) of
    sample.priortransform_batch: ``floor + gain A exp(-0.5 ((mu - x) / sig)^2)`` -- no floor: the background carries the
    rest --, every curve computed by itself."""
    x = np.ascontiguousarray(x, dtype=float)

    def model(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        out = np.empty((len(xs), len(x)))
        for k in range(len(xs)):
            out[k] = floor + gain * xs[k, 0] * np.exp(-0.5 * ((xs[k, 1] - x) / 10.0 ** xs[k, 2]) ** 2)
        return out
    return model


class DeviceScorer(object):
    """``loglike_batch(curves, mask)`` of a like.CountSpectra handle with a background: the kernel itself, for a numpy
    joint state."""

    def __init__(self, spectra):
        self.spectra = spectra

    def loglike_batch(self, curves, data_mask=None):
        return self.spectra.loglike_batch_curves(curves, data_mask)
