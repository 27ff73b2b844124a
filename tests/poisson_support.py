"""Test helper for the Poisson likelihood of count spectra (tests/test_poisson_curves_host.py,
tests/test_poisson_curves.py): low-count data with exposures and bad pixels, the numpy statement of the likelihood, the
float64 emulation of the kernel's chain, and the bound between the two.

The statement (include/mdns.h Part 10), with tiny = DBL_MIN and c' = c for c >= 0, NaN otherwise:

    L = sum_j ( n_j log(max(c'_j, tiny)) - e_j c'_j ) + K,     K = sum over n > 0, e > 0 of n (1 + log e - log n)

The chain (csrc/mdns_curves.hip, k_curve_log + k_curve_rows_p), per (curve, spectrum) pair, channels ascending, acc = +0:

    lc = log(fmax(c', tiny))   (once per candidate and channel);
    acc = fma(n, lc, acc);   acc = fma(-e, c', acc);          L = acc + K   (K: the statement's, rounded to float64)

The bound.  u = 2**-53, every rounding |delta| <= u.  The computed logarithm is lc^ = lc (1 + eps), |eps| <= lam =
LOG_ULPS 2**-52 (an error of so many ulps is at most that, relatively).  The products inside the fmas are exact, so the
2 nx terms t_1 = n_1 lc^_1, t_2 = -e_1 c'_1, ... enter a running sum that rounds once per fma, and the last addition of
K^ = K (1 + delta_K) rounds once more:

    L^ = sum_i t_i prod_(m >= i) (1 + delta_m) + K (1 + delta_K)(1 + delta_last)

with at most 2 nx + 1 factors behind any term.  Hence

    |L^ - L| <= ((1 + u)^(2 nx + 1) - 1) (sum_i |t_i| + |K|)  +  lam sum_j n_j |lc_j| (1 + u)^(2 nx + 1)
             <= (2 nx + 2) u S + lam sum_j n_j |lc_j| + (a cross term below (2 nx + 2) u lam S),
    S = sum_j (n_j |lc_j| + e_j c'_j) + |K|,

for every nx below 2**25.  The cross term is < 2**-40 u S for the sizes here; the statement itself is evaluated in
np.longdouble (64-bit significand on x86), whose own error -- (2 nx + 2) 2**-64 S and a 2**-63 relative error of its
logarithms -- is 2**-10 of the bound's.  Both live in the step from 2 nx + 2 to 2 nx + 4:

    bound = (2 nx + 4) 2**-53 S + LOG_ULPS 2**-52 sum_j n_j |lc_j|

LOG_ULPS.  HIP's table of math-function accuracy gives 1 ulp for the fp64 ``log`` (the ROCm documentation; no copy of it
ships with the toolkit, so the figure is an assumption here -- DESIGN section 4 says so); the table reports a sampled
maximum, not a proof, so the tests take twice that."""
import math
from fractions import Fraction

import numpy as np

from massivedatans_amd.like import count_pixels

U = 2.0 ** -53
TINY = np.finfo(np.float64).tiny                     # DBL_MIN
LOG_ULPS_DOCUMENTED = 1
LOG_ULPS = 2 * LOG_ULPS_DOCUMENTED


def bound(nx, S, nlc):
    """|L - L_statement| <= bound (module docstring): ``S`` = sum (n |lc| + e c') + |K|, ``nlc`` = sum n |lc|."""
    return (2 * nx + 4) * U * S + LOG_ULPS * 2.0 ** -52 * nlc


def count_data(ndata, nx, seed=0, exposure=True, edges=True):
    """Count spectra from a stream of their own, ``RandomState([seed, ndata, nx])``: per spectrum a level between 0.05
    and 50 counts per pixel (log-uniform) under a line of its own, Poisson counts at ``exposure`` e uniform in
    [0.5, 2] with 5 % planted zeros (``exposure=False``: none given, e = 1), 1 % of the counts NaN (bad pixels); and
    -- ``edges``, from three spectra on -- spectrum ``ndata // 3`` all zeros and spectrum ``2 * ndata // 3`` fully masked.
    Returns dict(x, y, e) with y, e of shape [nx, ndata] (e None without exposures)."""
    rng = np.random.RandomState([seed, ndata, nx])
    x = np.linspace(400.0, 800.0, nx)
    level = 10 ** rng.uniform(np.log10(0.05), np.log10(50.0), size=ndata)
    mu, sig = rng.uniform(450, 750, size=ndata), rng.uniform(5, 60, size=ndata)
    rate = level[None, :] * 0.5 * (1 + np.exp(-0.5 * ((x[:, None] - mu[None, :]) / sig[None, :]) ** 2))
    e = rng.uniform(0.5, 2.0, size=rate.shape)
    e[rng.uniform(size=rate.shape) < 0.05] = 0.0
    if not exposure:
        e = np.ones_like(rate)
    y = rng.poisson(rate * e).astype(float)
    y[rng.uniform(size=rate.shape) < 0.01] = np.nan
    if edges and ndata >= 3:
        y[:, ndata // 3] = 0.0
        if exposure:
            e[:, 2 * ndata // 3] = 0.0
        else:
            y[:, 2 * ndata // 3] = np.nan
    return dict(x=x, y=y, e=e if exposure else None)


class NumpyPoisson(object):
    """``loglike_batch(curves[B, nx], mask)``: the statement over counts ``y`` and exposures ``e`` (None: ones) of shape
    [nx, ndata], with the masking rule and the float64 offsets of like.count_pixels.  ``loglike_batch_long``: the same
    in np.longdouble with the offsets not rounded.  ``sums_long``: (S, sum n |lc|) of every pair, for ``bound``."""

    def __init__(self, y, e=None):
        self.y, self.e, self.masked, self.K = count_pixels(y, e)
        self.ndata = self.y.shape[1]
        self.n_masked = self.masked.sum(axis=0)
        good = self.y > 0
        n, ee = np.where(good, self.y, 1.0).astype(np.longdouble), np.where(good, self.e, 1.0).astype(np.longdouble)
        self.K_long = np.where(good, n * (1 + np.log(ee) - np.log(n)), np.longdouble(0)).sum(axis=0)
        assert np.array_equal(self.K_long.astype(np.float64), self.K)

    def _parts(self, curves, data_mask, dtype):
        c = np.atleast_2d(np.asarray(curves, dtype=float))
        c = np.where(c >= 0, c, np.nan).astype(dtype)
        with np.errstate(invalid="ignore"):
            lc = np.log(np.fmax(c, dtype(TINY)))
        sel = slice(None) if data_mask is None else np.asarray(data_mask)
        K = (self.K if dtype is np.float64 else self.K_long)[sel]
        return c, lc, self.y[:, sel].astype(dtype), self.e[:, sel].astype(dtype), K

    def _sum(self, curves, data_mask, dtype):
        c, lc, y, e, K = self._parts(curves, data_mask, dtype)
        out = np.empty((len(c), y.shape[1]), dtype=dtype)
        with np.errstate(invalid="ignore"):
            for b in range(len(c)):
                out[b] = (y * lc[b][:, None] - e * c[b][:, None]).sum(axis=0) + K
        return out

    def loglike_batch(self, curves, data_mask=None):
        return self._sum(curves, data_mask, np.float64)

    def loglike_batch_long(self, curves, data_mask=None):
        return self._sum(curves, data_mask, np.longdouble)

    def sums_long(self, curves, data_mask=None):
        c, lc, y, e, K = self._parts(curves, data_mask, np.longdouble)
        S, nlc = (np.empty((len(c), y.shape[1]), dtype=np.longdouble) for _ in range(2))
        with np.errstate(invalid="ignore"):
            for b in range(len(c)):
                nlc[b] = (y * np.abs(lc[b])[:, None]).sum(axis=0)
                S[b] = nlc[b] + (e * c[b][:, None]).sum(axis=0) + np.abs(K)
        return S, nlc


def within_bound(got, statement, nx, curves, data_mask=None, whole=None):
    """``(ok, worst)``: whether every ``got`` [B, M] lies within ``bound`` of ``statement.loglike_batch_long`` (a NaN
    exactly where the statement has one), and the largest error in units of the bound.  ``whole``: (statement, S,
    sum n |lc|) over ALL spectra, computed once by the caller; the selection's columns are taken from it."""
    if whole is None:
        want = statement.loglike_batch_long(curves, data_mask)
        S, nlc = statement.sums_long(curves, data_mask)
    else:
        want, S, nlc = (a if data_mask is None else a[:, np.asarray(data_mask)] for a in whole)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    lim = bound(nx, S[~nan].astype(float), nlc[~nan].astype(float))
    err = np.abs(got[~nan].astype(np.longdouble) - want[~nan]).astype(float)
    zero = lim == 0
    if (err[zero] != 0).any():
        return False, np.inf
    worst = float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0
    return worst <= 1.0, worst


def _fma(a, b, c):
    """fma(a, b, c): the exact a b + c, rounded once.  ``math.fma`` where Python has it; otherwise through Fraction
    (Fraction -> float rounds correctly), a non-finite operand through plain arithmetic (the result is NaN or an
    infinity either way)."""
    if hasattr(math, "fma"):
        try:
            return math.fma(a, b, c)
        except (ValueError, OverflowError):           # (math.fma raises where IEEE gives NaN or an infinity)
            return a * b + c
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def staged(curve):
    """What k_curve_log makes of one curve, with numpy's ``log``: ``(lc, c')`` f64[nx]."""
    c = np.asarray(curve, dtype=float)
    cp = np.where(c >= 0, c, np.nan)
    return np.log(np.fmax(cp, TINY)), cp


def chain(c, n, e, K, lc=None):
    """The kernel's chain for one pair in float64, operation by operation: curve ``c``, counts ``n``, exposures ``e``
    f64[nx] as uploaded (count_pixels), offset ``K``.  ``lc``: the logarithms to use (the device's own, for a bit-for-bit
    comparison); default numpy's."""
    lc0, cp = staged(c)
    lc = lc0 if lc is None else np.asarray(lc, dtype=float)
    acc = 0.0
    for l, cc, nn, ee in zip(lc.tolist(), cp.tolist(), np.asarray(n, dtype=float).tolist(), np.asarray(e, dtype=float).tolist()):
        acc = _fma(nn, l, acc)
        acc = _fma(-ee, cc, acc)
    return acc + float(K)


def count_model(x, gain=40.0, floor=0.05):
    """``model(xs[B, 3]) -> curves[B, nx]``, count rates > 0 for rows (A, mu, log10 sig) of sample.priortransform_batch:
    ``floor + gain A exp(-0.5 ((mu - x) / sig)^2)``, every curve computed by itself."""
    x = np.ascontiguousarray(x, dtype=float)

    def model(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        out = np.empty((len(xs), len(x)))
        for b in range(len(xs)):
            out[b] = floor + gain * xs[b, 0] * np.exp(-0.5 * ((xs[b, 1] - x) / 10.0 ** xs[b, 2]) ** 2)
        return out
    return model


class DeviceScorer(object):
    """``loglike_batch(curves, mask)`` of a like.CountSpectra handle: the kernel itself, for a numpy joint state."""

    def __init__(self, spectra):
        self.spectra = spectra

    def loglike_batch(self, curves, data_mask=None):
        return self.spectra.loglike_batch_curves(curves, data_mask)
