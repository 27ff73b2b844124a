"""Test helper for the fixed-scale chi^2 with per-pixel variances (tests/test_chi2_curves_host.py,
tests/test_chi2_curves.py): data with measured error bars and bad pixels, the numpy statement of the likelihood, the
float64 emulation of the kernel's chain, and the bound between the two.

The chain (csrc/mdns_curves.hip, k_curve_rows_w), per (curve, spectrum) pair, channels ascending, acc = +0:

    d = c - y;   t = w * d;   acc = fma(t, d, acc);          L = -0.5 * acc

The bound.  With u = 2**-53 and |delta| <= u for every rounding: d^ = d (1 + delta_1), t^ = w d^ (1 + delta_2), and the
product inside the fma is exact, so a channel's term enters the sum as w d^2 (1 + delta_1)^2 (1 + delta_2): three
roundings.  The running sum rounds once per fma, so the first channel's term passes through nx more roundings, every
later one through fewer.  All terms are >= 0 (w >= 0), so nothing cancels and the relative error of the sum is at most
that of its worst term: (1 + u)^(nx + 3) - 1 <= (nx + 3) u / (1 - (nx + 3) u) <= (nx + 4) u for every nx below 2**26.
The factor -0.5 is exact.  The statement itself is evaluated in np.longdouble (64-bit significand on x86: its own
error (nx + 3) 2**-64 is 2**-11 of that and lives in the slack between nx + 3 and nx + 4 for nx <= 2000)."""
from fractions import Fraction

import numpy as np

from massivedatans_amd import gen
from massivedatans_amd.like import mask_pixels

U = 2.0 ** -53


def rel_bound(nx):
    """|L - L_statement| <= rel_bound(nx) * |L_statement| (module docstring)."""
    return (nx + 4) * U


def weighted_data(ndata, nx, seed=0, masked=False):
    """``gen.horns(ndata)`` cut to ``nx`` channels (beyond its 200 the channels repeat), with a per-pixel sigma of
    0.01 (1 + 3 u), u uniform from ``RandomState(seed)``: the spectra carry sigma = 0.01 already, the rest is added.
    ``masked``: 5 % of the pixels are bad -- v = inf, y = NaN.  Returns dict(x, y, v) with y, v of shape [nx, ndata]."""
    d = gen.horns(ndata)
    rng = np.random.RandomState([seed, ndata, nx])
    y = np.ascontiguousarray(np.resize(d["y"], (nx, ndata)) if nx > 200 else d["y"][:nx])
    x = np.linspace(400, 800, nx) if nx > 200 else np.ascontiguousarray(d["x"][:nx])
    sigma = 0.01 * (1 + 3 * rng.uniform(size=y.shape))
    y = y + np.sqrt(sigma ** 2 - 0.01 ** 2) * rng.normal(size=y.shape)
    v = sigma ** 2
    if masked:
        bad = rng.uniform(size=y.shape) < 0.05
        y[bad] = np.nan
        v[bad] = np.inf
    return dict(x=x, y=y, v=v)


class NumpyWeightedChi2(object):
    """``loglike_batch(curves[B, nx], mask)``: -0.5 sum_j w_j (c_j - y_j)^2 over ``y``, ``v`` of shape [nx, ndata], with
    the masking rule and the float64 weights w = 1 / v of like.WeightedSpectra.  ``loglike_batch_long``: the same in
    np.longdouble, from the same float64 ``w``."""

    def __init__(self, y, v):
        self.y, v, self.masked = mask_pixels(y, v)
        self.w = 1.0 / v
        self.ndata = self.y.shape[1]
        self.n_masked = self.masked.sum(axis=0)

    def _sum(self, curves, data_mask, dtype):
        c = np.atleast_2d(np.asarray(curves, dtype=float)).astype(dtype)
        sel = slice(None) if data_mask is None else np.asarray(data_mask)
        y, w = self.y[:, sel].astype(dtype), self.w[:, sel].astype(dtype)
        out = np.empty((len(c), y.shape[1]), dtype=dtype)
        for b in range(len(c)):
            out[b] = (w * (c[b][:, None] - y) ** 2).sum(axis=0)
        return -0.5 * out

    def loglike_batch(self, curves, data_mask=None):
        return self._sum(curves, data_mask, np.float64)

    def loglike_batch_long(self, curves, data_mask=None):
        return self._sum(curves, data_mask, np.longdouble)


def _fma(a, b, c):
    """fma(a, b, c) of finite doubles: the exact a b + c, rounded once (Fraction -> float rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chain(curve, y, w):
    """The kernel's chain for one pair in float64, operation by operation: ``curve``, ``y``, ``w`` f64[nx]."""
    acc = 0.0
    for c, yy, ww in zip(np.asarray(curve, dtype=float).tolist(), np.asarray(y, dtype=float).tolist(), np.asarray(w, dtype=float).tolist()):
        d = c - yy
        acc = _fma(ww * d, d, acc)
    return -0.5 * acc


class DeviceScorer(object):
    """``loglike_batch(curves, mask)`` of a like.WeightedSpectra handle: the kernel itself, for a numpy joint state."""

    def __init__(self, spectra):
        self.spectra = spectra

    def loglike_batch(self, curves, data_mask=None):
        return self.spectra.loglike_batch_curves(curves, data_mask)
