"""A model that ships with the project: a sum of components, evaluated on the device.

Real analyses fit sums -- ``absorption x (power law + Fe line) + scattered table``, ``population A + population B +
emission line``.  :class:`SumModel` holds 1 to 8 components, each a :class:`massivedatans_amd.tablemodel.TableModel`, a
:class:`PowerLaw` or a :class:`GaussianLine`, and optionally one common attenuation factor ``10 ** (attenuation * N)``.
Given to :class:`massivedatans_amd.problem.CurveProblem` as its ``model``, the curves of every chunk are made on the GPU
from the candidates' parameters (``include/mdns.h`` Part 14, ``csrc/mdns_sum.hip``) and scored where they lie -- no
model function runs in Python and no curve crosses to the host.

    from massivedatans_amd import problem, sample
    from massivedatans_amd.summodel import SumModel, PowerLaw, GaussianLine

    # att x (power law + line) + a scattered table that the absorber does not see
    sm = SumModel([PowerLaw(x0=1.0), GaussianLine(), tm_scatter], attenuation=att, unattenuated=[2])
    p = problem.CurveProblem(channels, counts, sm, priortransform_batch, ndim=sm.ndim, poisson=True, exposure=t,
                             response=rsp)
    results, sampler, p, seconds = sample.run_model(p, nlive_points=400)

A candidate's row is the components' parameters one after the other in the order of the list (``sm.slices``) -- a table's
``(p_1 .. p_d [, z] [, E] [, s] [, A])``, a power law's ``(logA, G)``: ``10 ** logA * (x / x0) ** -G``, a line's
``(A, mu, sigma)``: ``A * exp(-0.5 ((x - mu) / sigma) ** 2)`` -- and, with an attenuation, ``N`` at the end.

:meth:`SumModel.statement` is the same chain of single rounded float64 operations in numpy: the CPU path, and what the
device agrees with bit for bit.  Its ``10 ** v`` is ``_host.pow10_dd``, the function the device computes
(csrc/mdns_pow10.h), which needs ``libmdns_host.so``.
"""
import numpy

from . import _host, _lib
from .tablemodel import BROADEN_C, MAX_DIM, TableModel, _clamp

MAX_COMPONENTS = _lib.SUM_MAX_COMPONENTS      # include/mdns.h MDNS_SUM_MAX_COMPONENTS


def _pow10(q):
    """``pow10_dd`` of a clamped exponent; a NaN (of a row that is NaN in the end) goes in as 0."""
    return _host.pow10_dd(numpy.where(numpy.isnan(q), 0.0, q))


class PowerLaw(object):
    """``10 ** logA * (x / x0) ** -G``: parameters ``(logA, G)``.  Needs ``x > 0``."""
    ndim = 2

    def __init__(self, x0=1.0):
        self.x0 = float(x0)
        if not (self.x0 > 0 and numpy.isfinite(self.x0)):
            raise ValueError("x0 = %r: the pivot of a power law must be finite and > 0" % (x0,))

    def lx(self, x):
        """``log10(x / x0)``, made once: the array both the statement and the device read."""
        x = numpy.ascontiguousarray(x, dtype=float)
        if not (x > 0).all():
            raise ValueError("a power law needs x > 0: x[%d] = %g" % (int(numpy.flatnonzero(~(x > 0))[0]), x[~(x > 0)][0]))
        return numpy.ascontiguousarray(numpy.log10(x / self.x0))

    def bad(self, p):
        return ~numpy.isfinite(p).all(axis=1)

    def values(self, x, p):
        q = p[:, 1, None] * self.lx(x)[None, :]
        q = p[:, 0, None] - q
        return _pow10(_clamp(q, -299.0, 299.0))


class GaussianLine(object):
    """``A * exp(-0.5 ((x - mu) / sigma) ** 2)``, the peak amplitude as in the reference's line: parameters
    ``(A, mu, sigma)``.  Not cut: far from the line the value is ``A * 1e-299``."""
    ndim = 3

    def bad(self, p):
        return ~(numpy.isfinite(p).all(axis=1) & (p[:, 2] > 0))

    def values(self, x, p):
        d = (x[None, :] - p[:, 1, None]) / p[:, 2, None]
        q = (BROADEN_C * d) * d
        return p[:, 0, None] * _pow10(_clamp(q, -299.0, 299.0))


class SumModel(object):
    """``components``: 1 to 8 of :class:`TableModel`, :class:`PowerLaw`, :class:`GaussianLine`; ``attenuation``
    f64[nx] (finite), the exponent per unit ``N`` at every bin of the abscissa the model is evaluated on: the sum of the
    attenuated components is multiplied by ``10 ** (attenuation * N)`` and ``N`` is the last parameter;
    ``unattenuated``: the indices of the components that factor does not touch.  ``ndim``: the components' parameters,
    plus 1 with an attenuation; ``slices[c]``: where component ``c``'s parameters stand in a row."""

    def __init__(self, components, attenuation=None, unattenuated=()):
        try:
            components = list(components)
        except TypeError:
            raise ValueError("components must be a sequence of TableModel, PowerLaw and GaussianLine objects")
        if not 1 <= len(components) <= MAX_COMPONENTS:
            raise ValueError("%d components: 1 to %d" % (len(components), MAX_COMPONENTS))
        for k, c in enumerate(components):
            if not isinstance(c, (TableModel, PowerLaw, GaussianLine)):
                raise ValueError("component %d is a %s: TableModel, PowerLaw or GaussianLine" % (k, type(c).__name__))
        self.components = components
        self.att = None
        if attenuation is not None:
            self.att = numpy.ascontiguousarray(attenuation, dtype=float)
            if self.att.ndim != 1:
                raise ValueError("attenuation must be a one-dimensional array, got shape %s" % (self.att.shape,))
            if not numpy.isfinite(self.att).all():
                raise ValueError("attenuation[%d] is not finite" % int(numpy.flatnonzero(~numpy.isfinite(self.att))[0]))
        free = set()
        for k in unattenuated:
            if int(k) != k or not 0 <= k < len(components):
                raise ValueError("unattenuated holds %r: the indices of the %d components" % (k, len(components)))
            free.add(int(k))
        # (without an attenuation every component counts as attenuated: one sum, in the order of the list)
        self.attenuated = [self.att is None or k not in free for k in range(len(components))]
        self.slices, at = [], 0
        for c in components:
            self.slices.append(slice(at, at + c.ndim))
            at += c.ndim
        self.ndim = at + (0 if self.att is None else 1)
        if self.ndim > MAX_DIM:
            raise ValueError("%d parameters: %d at most" % (self.ndim, MAX_DIM))

    def _abscissa(self, x):
        x = numpy.ascontiguousarray(x, dtype=float)
        if x.ndim != 1 or len(x) < 1:
            raise ValueError("x must be a one-dimensional array, got shape %s" % (x.shape,))
        if self.att is not None and len(self.att) != len(x):
            raise ValueError("attenuation has %d values, x has %d" % (len(self.att), len(x)))
        for c in self.components:
            if isinstance(c, PowerLaw):
                c.lx(x)                                                   # (x > 0, or its ValueError)
        return x

    def statement(self, x, xs):
        """``xs[B, ndim] -> curves[B, nx]`` on the abscissa ``x``: include/mdns.h Part 14 in numpy, vectorised over the
        candidates, every step one rounded float64 operation in the kernel's order."""
        x = self._abscissa(x)
        xs = numpy.atleast_2d(numpy.asarray(xs, dtype=float))
        if xs.ndim != 2 or xs.shape[1] != self.ndim:
            raise ValueError("xs must be [B, %d], got %s" % (self.ndim, xs.shape))
        B = len(xs)
        bad = numpy.isnan(xs).any(axis=1)
        a, u = numpy.zeros((B, len(x))), numpy.zeros((B, len(x)))
        with numpy.errstate(all="ignore"):
            for c, sl, attenuated in zip(self.components, self.slices, self.attenuated):
                p = xs[:, sl]
                if isinstance(c, TableModel):
                    v = c.statement(x, p)
                else:
                    bad |= c.bad(p)
                    v = c.values(x, p)
                if attenuated:
                    a = a + v
                else:
                    u = u + v
            if self.att is not None:
                N = xs[:, -1]
                bad |= ~numpy.isfinite(N)
                a = a * _pow10(_clamp(self.att[None, :] * N[:, None], -299.0, 299.0))
            out = a + u
        out[bad] = numpy.nan
        return out

    def bind(self, x):
        """The model on the GPU for curves on the abscissa ``x``: a :class:`DeviceSum` (close it, or drop it)."""
        return DeviceSum(self, x)


class DeviceSum(object):
    """A :class:`SumModel` bound to an abscissa and resident on the device (``mdns_sum_create`` and its add entries; the
    handle owns its tables).  ``handle`` goes to ``mdns_backend_draw_sum`` / ``mdns_joint_init_sum`` -- the two entries a
    :class:`massivedatans_amd.jointstate.CurveJointState` reads off ``init_entry`` / ``draw_entry`` --; :meth:`curves`
    fetches curves to the host."""
    init_entry, draw_entry = "mdns_joint_init_sum", "mdns_backend_draw_sum"

    def __init__(self, model, x):
        self._h = None
        x = model._abscissa(x)
        self._lib = _lib.require_device()
        self._h = self._lib.mdns_sum_create(_lib.ptr(x), len(x))
        if not self._h:
            raise _lib.MdnsError("mdns_sum_create failed: " + _lib.last_error())
        try:
            for c, attenuated in zip(model.components, model.attenuated):
                if isinstance(c, TableModel):
                    n = numpy.array([len(a) for a in c.axes], dtype=numpy.int32)
                    axes = numpy.ascontiguousarray(numpy.concatenate(c.axes))
                    rc = self._lib.mdns_sum_add_table(self._h, c.d, _lib.ptr(n), _lib.ptr(axes), len(c.grid), _lib.ptr(c.grid),
                                                      _lib.ptr(c.table), c.flags, _lib.ptr(c.ext) if c.extinction else None,
                                                      int(attenuated))
                    _lib.check(rc, "mdns_sum_add_table")
                elif isinstance(c, PowerLaw):
                    lx = c.lx(x)
                    _lib.check(self._lib.mdns_sum_add_powerlaw(self._h, _lib.ptr(lx), int(attenuated)), "mdns_sum_add_powerlaw")
                else:
                    _lib.check(self._lib.mdns_sum_add_gauss(self._h, int(attenuated)), "mdns_sum_add_gauss")
            if model.att is not None:
                _lib.check(self._lib.mdns_sum_set_attenuation(self._h, _lib.ptr(model.att)), "mdns_sum_set_attenuation")
        except Exception:
            self.close()
            raise
        self.model, self.nx, self.ndim = model, len(x), model.ndim

    @property
    def handle(self):
        if not self._h:
            raise _lib.MdnsError("the sum model was closed")
        return self._h

    def curves(self, xs):
        """``xs[B, ndim] -> curves[B, nx]`` made on the device (mdns_sum_curves_batch)."""
        xs = numpy.atleast_2d(_lib.as_f64(xs))
        if xs.shape[1] != self.ndim:
            raise ValueError("xs must be [B, %d], got %s" % (self.ndim, xs.shape))
        out = numpy.empty((len(xs), self.nx))
        _lib.check(self._lib.mdns_sum_curves_batch(self.handle, _lib.ptr(xs), len(xs), _lib.ptr(out)), "mdns_sum_curves_batch")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mdns_sum_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


__all__ = ['SumModel', 'PowerLaw', 'GaussianLine', 'DeviceSum']
