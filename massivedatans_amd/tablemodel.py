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

:meth:`TableModel.statement` is the same chain of single rounded float64 operations in numpy: the CPU path, and what
the device agrees with bit for bit.
"""
import numpy

from . import _lib

MAX_AXES = _lib.TABLE_MAX_AXES                # include/mdns.h MDNS_TABLE_MAX_AXES
MAX_DIM = 16                                  # include/mdns.h MDNS_MAX_DIM


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
    ``(p_1 ... p_d [, z] [, A])``: ``z`` with ``redshift=True`` (the template is read at ``x / (1 + z)``), ``A`` with
    ``amplitude=True`` (the curve is multiplied by it).  Linear interpolation everywhere; outside an axis or the grid
    the end value holds (``numpy.interp``'s rule)."""

    def __init__(self, axes, grid, table, redshift=False, amplitude=False):
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
        self.redshift, self.amplitude = bool(redshift), bool(amplitude)
        self.ndim = self.d + int(self.redshift) + int(self.amplitude)
        if self.ndim > MAX_DIM:
            raise ValueError("%d parameters: %d at most" % (self.ndim, MAX_DIM))
        self.flags = (_lib.TABLE_REDSHIFT if self.redshift else 0) | (_lib.TABLE_AMPLITUDE if self.amplitude else 0)

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
            acc = numpy.zeros((B, len(x)))
            for c in range(1 << d):
                lo, hi = rows[row[:, c, None], k], rows[row[:, c, None], k + 1]
                acc = acc + w[:, c, None] * (lo + t * (hi - lo))
            if self.amplitude:
                acc = xs[:, -1, None] * acc
        acc[numpy.isnan(xs).any(axis=1)] = numpy.nan
        return acc

    def bind(self, x):
        """The table on the GPU for curves on the abscissa ``x``: a :class:`DeviceTable` (close it, or drop it)."""
        return DeviceTable(self, x)


class DeviceTable(object):
    """A :class:`TableModel` bound to an abscissa and resident on the device (``mdns_table_create``).  ``handle`` goes
    to ``mdns_backend_draw_table`` / ``mdns_joint_init_table``; :meth:`curves` fetches curves to the host."""

    def __init__(self, model, x):
        self._lib = _lib.require_device()
        self._h = None
        x = numpy.ascontiguousarray(x, dtype=float)
        if x.ndim != 1 or len(x) < 1:
            raise ValueError("x must be a one-dimensional array, got shape %s" % (x.shape,))
        n = numpy.array([len(a) for a in model.axes], dtype=numpy.int32)
        axes = numpy.ascontiguousarray(numpy.concatenate(model.axes))
        self._h = self._lib.mdns_table_create(_lib.ptr(x), len(x), model.d, _lib.ptr(n), _lib.ptr(axes), len(model.grid),
                                              _lib.ptr(model.grid), _lib.ptr(model.table), model.flags)
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
