"""A model that ships with the project: a grid of tabulated templates, interpolated on the device.

The reference's real workload computes its model this way (musefuse.py:222-284): templates tabulated over a few
parameters, interpolated in the grid's parameters and resampled at ``wavelength / (1 + z)`` with ``numpy.interp``; X-ray
fitters ship physical models as such tables too.  :class:`TableModel` holds the table; given to
:class:`massivedatans_amd.problem.CurveProblem` as its ``model``, the curves of every chunk are made on the GPU from the
candidates' parameters (``include/mdns.h`` Part 12, ``csrc/mdns_table.hip``) and scored where they lie -- no model
function runs in Python and no curve crosses to the host.

    import numpy
    from massivedatans_amd import problem, sample
    from massivedatans_amd.tablemodel import TableModel

    # table[n_age, n_metal, nw]: one template per (age, metallicity) on the rest-frame wavelengths `grid`
    tm = TableModel([ages, metals], grid, table, redshift=True, amplitude=True)    # xs rows: (age, metal, z, A)

    def priortransform_batch(us):
        return numpy.column_stack((ages[0] + (ages[-1] - ages[0]) * us[:, 0], metals[0] + (metals[-1] - metals[0]) * us[:, 1],
                                   0.1 * us[:, 2], 10 ** (2 * us[:, 3] - 1)))

    p = problem.CurveProblem(x, y, tm, priortransform_batch, ndim=tm.ndim, v=v, marginalise_scale=False)
    results, sampler, p, seconds = sample.run_model(p, nlive_points=400)

Two line-of-sight effects are parameters as well: ``extinction=ext`` adds ``E`` (the blended template is multiplied by
``10 ** (ext * E)`` knot by knot; pass e.g. ``-0.4 * k(wavelength)`` for a reddening law ``k``), ``broadening=True`` adds
``s``, a velocity dispersion as sigma_v / c (the template is convolved with a Gaussian in velocity before it is
resampled).  A candidate is then ``(p_1 .. p_d [, z] [, E] [, s] [, A])``.  The Gaussian's window is 5 sigma and has no
cap in knots: a large ``s`` on a dense grid costs O(nw) per template knot.

:meth:`TableModel.statement` is the same chain of single rounded float64 operations in numpy: the CPU path, and what
the device agrees with bit for bit.  With either line-of-sight effect its ``10 ** v`` is ``_host.pow10_dd``, the function
the device computes (csrc/mdns_pow10.h), which needs ``libmdns_host.so``.
"""
import numpy

from . import _host, _lib

MAX_AXES = _lib.TABLE_MAX_AXES                # include/mdns.h MDNS_TABLE_MAX_AXES
MAX_DIM = 16                                  # include/mdns.h MDNS_MAX_DIM
BROADEN_CUT = _lib.TABLE_BROADEN_CUT          # include/mdns.h MDNS_TABLE_BROADEN_CUT
BROADEN_C = _lib.TABLE_BROADEN_C              # include/mdns.h MDNS_TABLE_BROADEN_C


def _knots(a, what):
    a = numpy.ascontiguousarray(a, dtype=float)
    if a.ndim != 1 or len(a) < 2:
        raise ValueError("%s must be a one-dimensional array of 2 knots at least, got shape %s" % (what, a.shape))
    if not numpy.isfinite(a).all():
        raise ValueError("%s holds a value that is not finite" % what)
    if not (numpy.diff(a) > 0).all():
        raise ValueError("%s is not strictly increasing" % what)
    return a


def _clamp(v, lo, hi):
    """The statement's clamp, as comparisons: +-inf clamp, a NaN stays (fmin / fmax would drop it)."""
    return numpy.where(v < lo, lo, numpy.where(v > hi, hi, v))


def _last_knot(knots, v):
    """The last knot <= v, at most len(knots) - 2 (v >= knots[0], or NaN -- whose value is NaN whatever the cell)."""
    return numpy.clip(numpy.searchsorted(knots, v, side="right") - 1, 0, len(knots) - 2)


class TableModel(object):
    """``axes``: ``d`` arrays (1 to 4), each of 2 knots at least, finite and strictly increasing; ``grid`` f64[nw]
    likewise, the templates' own abscissa; ``table`` f64[n_1, ..., n_d, nw], finite.  A candidate is the row
    ``(p_1 ... p_d [, z] [, E] [, s] [, A])``: ``z`` with ``redshift=True`` (the template is read at ``x / (1 + z)``),
    ``E`` with ``extinction=ext`` (f64[nw], finite: the exponent per unit ``E`` at each knot of the grid), ``s`` with
    ``broadening=True`` (sigma_v / c; needs ``grid[0] > 0``), ``A`` with ``amplitude=True`` (the curve is multiplied by
    it).  Linear interpolation everywhere; outside an axis or the grid the end value holds (``numpy.interp``'s rule)."""

    def __init__(self, axes, grid, table, redshift=False, amplitude=False, extinction=None, broadening=False):
        try:
            axes = list(axes)
        except TypeError:
            raise ValueError("axes must be a sequence of one-dimensional arrays")
        if not 1 <= len(axes) <= MAX_AXES:
            raise ValueError("%d axes: 1 to %d" % (len(axes), MAX_AXES))
        self.axes = [_knots(a, "axis %d" % k) for k, a in enumerate(axes)]
        self.grid = _knots(grid, "grid")
        self.table = numpy.ascontiguousarray(table, dtype=float)
        shape = tuple(len(a) for a in self.axes) + (len(self.grid),)
        if self.table.shape != shape:
            raise ValueError("table has shape %s, axes and grid ask for %s" % (self.table.shape, shape))
        if self.table.size > 2 ** 31 - 1:
            raise ValueError("table of %d values: %d at most" % (self.table.size, 2 ** 31 - 1))
        if not numpy.isfinite(self.table).all():
            raise ValueError("table holds a value that is not finite")
        self.d = len(self.axes)
        self.redshift, self.amplitude, self.broadening = bool(redshift), bool(amplitude), bool(broadening)
        self.ext = None
        if extinction is not None:
            self.ext = numpy.ascontiguousarray(extinction, dtype=float)
            if self.ext.shape != self.grid.shape:
                raise ValueError("extinction has shape %s, the grid has %d knots" % (self.ext.shape, len(self.grid)))
            if not numpy.isfinite(self.ext).all():
                raise ValueError("extinction[%d] is not finite" % int(numpy.flatnonzero(~numpy.isfinite(self.ext))[0]))
        if self.broadening and not self.grid[0] > 0:
            raise ValueError("grid[0] = %g: broadening needs a grid > 0" % self.grid[0])
        self.extinction = self.ext is not None
        self.ndim = self.d + int(self.redshift) + int(self.extinction) + int(self.broadening) + int(self.amplitude)
        if self.ndim > MAX_DIM:
            raise ValueError("%d parameters: %d at most" % (self.ndim, MAX_DIM))
        self.flags = ((_lib.TABLE_REDSHIFT if self.redshift else 0) | (_lib.TABLE_AMPLITUDE if self.amplitude else 0) |
                      (_lib.TABLE_EXTINCTION if self.extinction else 0) | (_lib.TABLE_BROADEN if self.broadening else 0))
        # where E and s stand in a candidate's row
        self.at_e = self.d + int(self.redshift)
        self.at_s = self.at_e + int(self.extinction)
        # the quadrature widths of the broadening sum (mdns_table_create_los makes the same)
        g = self.grid
        self.delta = numpy.concatenate(([(g[1] - g[0]) * 0.5], (g[2:] - g[:-2]) * 0.5, [(g[-1] - g[-2]) * 0.5]))

    def statement(self, x, xs):
        """``xs[B, ndim] -> curves[B, nx]`` on the abscissa ``x``: include/mdns.h Part 12 in numpy, vectorised over the
        candidates, every step one rounded float64 operation in the kernel's order."""
        x = numpy.ascontiguousarray(x, dtype=float)
        xs = numpy.atleast_2d(numpy.asarray(xs, dtype=float))
        if x.ndim != 1 or xs.ndim != 2 or xs.shape[1] != self.ndim:
            raise ValueError("x must be [nx] and xs [B, %d], got %s and %s" % (self.ndim, x.shape, xs.shape))
        B, d, nw = len(xs), self.d, len(self.grid)
        rows = self.table.reshape(-1, nw)
        with numpy.errstate(all="ignore"):
            w = numpy.ones((B, 1 << d))
            row = numpy.zeros((B, 1 << d), dtype=numpy.int64)
            stride = 1
            strides = []
            for a in reversed(range(d)):
                strides.insert(0, stride)
                stride *= len(self.axes[a])
            for a, axis in enumerate(self.axes):
                v = _clamp(xs[:, a], axis[0], axis[-1])
                i = _last_knot(axis, v)
                f = (v - axis[i]) / (axis[i + 1] - axis[i])
                g = 1.0 - f
                for c in range(1 << d):
                    bit = (c >> a) & 1
                    w[:, c] = w[:, c] * (f if bit else g)
                    row[:, c] += (i + bit) * strides[a]
            u = numpy.broadcast_to(x, (B, len(x)))
            if self.redshift:
                u = u / (1.0 + xs[:, d, None])
            u = _clamp(u, self.grid[0], self.grid[-1])
            k = _last_knot(self.grid, u)
            g0 = self.grid[k]
            t = (u - g0) / (self.grid[k + 1] - g0)
            if self.extinction or self.broadening:
                acc = self._line_of_sight(xs, w, row, rows, k, t)
            else:
                acc = numpy.zeros((B, len(x)))
                for c in range(1 << d):
                    lo, hi = rows[row[:, c, None], k], rows[row[:, c, None], k + 1]
                    acc = acc + w[:, c, None] * (lo + t * (hi - lo))
            if self.amplitude:
                acc = xs[:, -1, None] * acc
        bad = numpy.isnan(xs).any(axis=1)
        if self.extinction:
            bad |= ~numpy.isfinite(xs[:, self.at_e])
        if self.broadening:
            bad |= ~(numpy.isfinite(xs[:, self.at_s]) & (xs[:, self.at_s] >= 0))
        acc[bad] = numpy.nan
        return acc

    def _line_of_sight(self, xs, w, row, rows, k, t):
        """Blend, attenuate, broaden, interpolate (include/mdns.h Part 12, "with either new flag"): ``[B, nx]`` before
        the amplitude.  ``w``, ``row`` [B, 2^d]: corner weights and table rows; ``k``, ``t`` [B, nx]: cell and
        fraction along the grid."""
        B, nw = len(xs), len(self.grid)
        S = numpy.zeros((B, nw))
        for c in range(w.shape[1]):
            S = S + w[:, c, None] * rows[row[:, c]]
        if self.extinction:
            q = _clamp(self.ext[None, :] * xs[:, self.at_e, None], -299.0, 299.0)
            q = numpy.where(numpy.isnan(q), 0.0, q)                       # (a NaN E: the row is NaN in the end)
            S = S * _host.pow10_dd(q)
        R = S
        if self.broadening:
            s = xs[:, self.at_s]
            wide = numpy.isfinite(s) & (s > 0)                            # rows that are summed; s == 0 keeps R = S
            if wide.any():
                R = S.copy()
                R[wide] = self._broaden(S[wide], s[wide])
        at = numpy.arange(B)[:, None]
        lo, hi = R[at, k], R[at, k + 1]
        return lo + t * (hi - lo)

    def _offset(self, o, s):
        """For the offset ``o = n - m``: the knots ``m`` that have a knot ``n``, d_mn [B, len(m)] and whether n is in
        the window of m."""
        g, nw = self.grid, len(self.grid)
        m = numpy.arange(max(0, -o), min(nw, nw - o))
        dmn = ((g[m + o] - g[m]) / g[m])[None, :] / s[:, None]
        return m, dmn, numpy.abs(dmn) <= BROADEN_CUT

    def _broaden(self, S, s):
        """R[B, nw] for rows with finite s > 0: per knot m the two running sums over its window, n ascending -- here a
        loop over the offset o = n - m from the most negative to the most positive that occurs, each step
        ``acc = acc + where(inside, term, 0.0)`` (adding +0.0 changes nothing), which is the kernel's order."""
        B, nw = S.shape
        # a window is a contiguous run around m, so an offset at which no (b, m) is inside ends the search on its side
        first, last = 0, 0
        while first - 1 > -nw and self._offset(first - 1, s)[2].any():
            first -= 1
        while last + 1 < nw and self._offset(last + 1, s)[2].any():
            last += 1
        num, den = numpy.zeros((B, nw)), numpy.zeros((B, nw))
        for o in range(first, last + 1):
            m, dmn, inside = self._offset(o, s)
            K = numpy.zeros(dmn.shape)
            K[inside] = _host.pow10_dd(((BROADEN_C * dmn) * dmn)[inside])
            K = K * self.delta[None, m + o]
            num[:, m] = num[:, m] + numpy.where(inside, S[:, m + o] * K, 0.0)
            den[:, m] = den[:, m] + numpy.where(inside, K, 0.0)
        return num / den

    def bind(self, x):
        """The table on the GPU for curves on the abscissa ``x``: a :class:`DeviceTable` (close it, or drop it)."""
        return DeviceTable(self, x)


class DeviceTable(object):
    """A :class:`TableModel` bound to an abscissa and resident on the device (``mdns_table_create``, with a line-of-sight
    effect ``mdns_table_create_los``).  ``handle`` goes to ``mdns_backend_draw_table`` / ``mdns_joint_init_table``;
    :meth:`curves` fetches curves to the host."""

    def __init__(self, model, x):
        self._lib = _lib.require_device()
        self._h = None
        x = numpy.ascontiguousarray(x, dtype=float)
        if x.ndim != 1 or len(x) < 1:
            raise ValueError("x must be a one-dimensional array, got shape %s" % (x.shape,))
        n = numpy.array([len(a) for a in model.axes], dtype=numpy.int32)
        axes = numpy.ascontiguousarray(numpy.concatenate(model.axes))
        args = (_lib.ptr(x), len(x), model.d, _lib.ptr(n), _lib.ptr(axes), len(model.grid), _lib.ptr(model.grid), _lib.ptr(model.table),
                model.flags)
        if model.extinction or model.broadening:
            self._h = self._lib.mdns_table_create_los(*(args + (_lib.ptr(model.ext) if model.extinction else None,)))
        else:
            self._h = self._lib.mdns_table_create(*args)
        if not self._h:
            raise _lib.MdnsError("mdns_table_create failed: " + _lib.last_error())
        self.model, self.nx, self.ndim = model, len(x), model.ndim

    @property
    def handle(self):
        if not self._h:
            raise _lib.MdnsError("the table was closed")
        return self._h

    def curves(self, xs):
        """``xs[B, ndim] -> curves[B, nx]`` made on the device (mdns_table_curves_batch)."""
        xs = numpy.atleast_2d(_lib.as_f64(xs))
        if xs.shape[1] != self.ndim:
            raise ValueError("xs must be [B, %d], got %s" % (self.ndim, xs.shape))
        out = numpy.empty((len(xs), self.nx))
        _lib.check(self._lib.mdns_table_curves_batch(self.handle, _lib.ptr(xs), len(xs), _lib.ptr(out)), "mdns_table_curves_batch")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mdns_table_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


__all__ = ['TableModel', 'DeviceTable']
