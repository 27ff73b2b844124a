"""Host side of the likelihood hot path: spectra resident in HBM, candidates scored in batches.

Mirrors the problem-definition surface of the reference driver scripts:

* :class:`GaussLineSpectra` -- ``multi_loglikelihood(params, data_mask)`` of sample.py:101-108
  (one Gaussian emission line; clike.c).
* :class:`MuseSpectra` -- ``multi_loglikelihood_clike`` of musefuse.py:520-535 (scale-marginalised
  chi^2 against a template; cmuselike.c), without the RNG jitter (callers add it, see
  ``jitter``).
* :class:`WeightedSpectra` -- per-pixel variances at fixed scale, for model curves the caller makes
  (:mod:`massivedatans_amd.problem`); no counterpart in the reference.
* :class:`CountSpectra` -- photon counts with per-pixel exposures, the Poisson likelihood for the same model curves, or
  -- with a background spectrum per spectrum -- the W statistic; no counterpart in the reference.

All keep the spectra on the device as ``[n_datasets, n_channels]`` rows and add
``loglike_batch`` (B candidates per pass), which the reference does not have.
"""
import ctypes as C

import numpy as np

from . import _lib


def _rows_from_mask(data_mask, ndata):
    """Ascending indices of the selected spectra (None = all of them)."""
    if data_mask is None:
        return None, ndata
    m = np.asarray(data_mask)
    if m.dtype == np.bool_:
        if m.shape != (ndata,):
            raise ValueError("data_mask has shape %s, expected (%d,)" % (m.shape, ndata))
        if m.all():
            return None, ndata
        rows = np.flatnonzero(m).astype(np.int32)
    else:
        rows = np.ascontiguousarray(m, dtype=np.int32)
    return rows, len(rows)


class _Spectra(object):
    def __init__(self, x, y, v=None, layout="channel_major"):
        self._lib = _lib.require_device()
        y = _lib.as_f64(y)
        if y.ndim != 2:
            raise ValueError("y must be 2-D")
        if layout == "channel_major":        # reference layout [nx, ndata] (sample.py:31)
            nx, ndata = y.shape
            code = 0
        elif layout == "dataset_major":
            ndata, nx = y.shape
            code = 1
        else:
            raise ValueError(layout)
        self.ndata, self.nx = int(ndata), int(nx)
        self._response = None
        xp = None
        if x is not None:
            x = _lib.as_f64(x)
            if x.shape != (nx,):
                raise ValueError("x has shape %s, expected (%d,)" % (x.shape, nx))
            xp = _lib.ptr(x)
        vp = None
        if v is not None:
            v = _lib.as_f64(v)
            if v.shape != y.shape:
                raise ValueError("v and y differ in shape")
            vp = _lib.ptr(v)
        self._h = self._lib.mdns_spectra_create(xp, _lib.ptr(y), vp, self.ndata, self.nx, code)
        if not self._h:
            raise _lib.MdnsError("mdns_spectra_create failed: " + _lib.last_error())

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mdns_spectra_destroy(self._h)           # (releases a response it had borrowed)
            self._h = None
            self._response = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def response(self):
        """The :class:`massivedatans_amd.response.DeviceResponse` attached to these spectra, or None."""
        return self._response

    @property
    def n_in(self):
        """Values per model curve: the bins of the attached response, or -- without one -- the channels."""
        return self.nx if self._response is None else self._response.n_in

    def set_response(self, response):
        """Attaches an instrument response (a :class:`massivedatans_amd.response.DeviceResponse`; a
        :class:`massivedatans_amd.response.Response` is bound first; None detaches): from now on every scoring on these
        spectra takes curves of ``response.n_in`` bins and folds them on the device first (include/mdns.h Part 13).
        The spectra keep the device response alive.  Refused (MdnsError) for a response of another ``nx`` and while a
        joint state lives on the spectra."""
        if response is not None and not hasattr(response, "handle"):
            response = response.bind()
        _lib.check(self._lib.mdns_spectra_set_response(self._h, None if response is None else response.handle),
                   "mdns_spectra_set_response")
        self._response = response

    def _batch(self, fn, name, params, data_mask, *extra):
        params = _lib.as_f64(params)
        B = params.shape[0]
        rows, M = _rows_from_mask(data_mask, self.ndata)
        out = np.empty((B, M))
        if B and M:
            args = [self._h, _lib.ptr(params), B] + list(extra) + \
                   [_lib.opt(rows), M, _lib.ptr(out)]
            _lib.check(fn(*args), name)
        return out

    def _curves_batch(self, name, curves, data_mask, *extra):
        """``curves[B, nx]`` (one curve: ``[nx]``; with a response ``[B, n_in]``, folded on the device) through the library's
        batch function ``name`` -> ``L[B, mask.sum()]``."""
        curves = np.atleast_2d(_lib.as_f64(curves))
        if curves.shape[1] != self.n_in:
            raise ValueError("curves must be [B, %d]" % self.n_in)
        return self._batch(getattr(self._lib, name), name, curves, data_mask, *extra)


class GaussLineSpectra(_Spectra):
    """The toy problem of sample.py: ``ypred = A exp(-0.5 ((mu - x)/sig)^2)``,
    ``L_i = -0.5 sum_j ((ypred_j - y_ji)/noise_level)^2``."""

    def __init__(self, x, y, noise_level=0.01, layout="channel_major"):
        super(GaussLineSpectra, self).__init__(x, y, None, layout)
        self.noise_level = float(noise_level)

    def loglike_batch(self, params, data_mask=None):
        """``params[B, 3]`` = (A, mu, sig) with sig linear -> ``L[B, mask.sum()]``."""
        params = np.atleast_2d(_lib.as_f64(params))
        if params.shape[1] != 3:
            raise ValueError("params must be [B, 3] = (A, mu, sig)")
        return self._batch(self._lib.mdns_gauss_loglike_batch, "mdns_gauss_loglike_batch",
                           params, data_mask, self.noise_level)

    def loglike_batch_curves(self, curves, data_mask=None):
        """``curves[B, nx]`` model curves the caller made, one per candidate (any model) ->
        ``L[B, mask.sum()]``, ``L = -0.5 sum_j ((curve_j - y_j) / noise_level)^2`` (sample.py:64-71)."""
        return self._curves_batch("mdns_curve_loglike_batch", curves, data_mask, self.noise_level)

    def multi_loglikelihood(self, params, data_mask):
        """Same call as sample.py:101-108: ``params = (A, mu, log10 sig)`` after
        priortransform; returns the likelihood vector of the masked data sets."""
        A, mu, log_sig = params
        sig = 10 ** log_sig
        return self.loglike_batch(np.array([[A, mu, sig]]), data_mask)[0]


def mask_pixels(y, v):
    """What :class:`WeightedSpectra` uploads for ``y``, ``v`` of one shape: ``(y, v, masked)``, copies in which a pixel
    whose ``v`` is ``inf`` or NaN, or whose ``y`` is not finite, is MASKED -- ``y = 0``, ``v = inf``, so that its weight
    ``1 / v`` is 0 and its residual finite -- and ``masked`` says which.  Any other ``v <= 0`` raises ValueError.  Needs
    no device."""
    y, v = np.array(y, dtype=np.float64), np.array(v, dtype=np.float64)
    if v.shape != y.shape:
        raise ValueError("v and y differ in shape")
    masked = np.isnan(v) | (v == np.inf) | ~np.isfinite(y)
    bad = ~masked & ~(v > 0)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise ValueError("v%s = %r: variances must be positive (inf or NaN masks a pixel)" % (list(at), float(v[at])))
    y[masked] = 0.0
    v[masked] = np.inf
    return y, v, masked


class WeightedSpectra(_Spectra):
    """Spectra with per-pixel variances scored at FIXED scale against model curves the caller made (include/mdns.h
    Part 9): ``L = -0.5 sum_j (curve_j - y_j)^2 / v_j``, nothing fitted per spectrum -- the model's amplitude is the
    caller's parameter.  A pixel with ``v`` ``inf`` or NaN, or a non-finite ``y``, is masked (:func:`mask_pixels`) and
    contributes nothing; ``n_masked`` [ndata] counts them per spectrum.  A joint state on these spectra
    (:class:`massivedatans_amd.jointstate.CurveJointState`) scores its curve chunks the same way."""

    def __init__(self, x, y, v, layout="channel_major"):
        if v is None:
            raise ValueError("WeightedSpectra needs the variances v")
        y, v, masked = mask_pixels(y, v)
        super(WeightedSpectra, self).__init__(x, y, v, layout)
        self.n_masked = masked.sum(axis=0 if layout == "channel_major" else 1)
        _lib.check(self._lib.mdns_spectra_set_fixed_scale(self._h, 1), "mdns_spectra_set_fixed_scale")

    def loglike_batch_curves(self, curves, data_mask=None):
        """``curves[B, nx]`` -> ``L[B, mask.sum()]`` (mdns_curve_chi2_batch)."""
        return self._curves_batch("mdns_curve_chi2_batch", curves, data_mask)

    loglike_batch = loglike_batch_curves


def count_pixels(y, e=None, axis=0):
    """What :class:`CountSpectra` uploads for counts ``y`` and exposures ``e`` of one shape (``e=None``: all ones):
    ``(y, e, masked, offsets)``, copies in which a pixel whose ``e`` is 0 or NaN, or whose ``y`` is not finite, is MASKED
    -- ``y = 0``, ``e = 0``, a deleted channel to the likelihood -- and ``masked`` says which.  On a pixel that is not
    masked ``y < 0``, ``e < 0`` and ``e = inf`` raise ValueError.  ``offsets`` [the other axis]: per spectrum the
    ``K = sum n (1 + log e - log n)`` over its pixels with ``n > 0`` and ``e > 0`` (``axis``: the channel axis; 0 in
    the reference's layout ``[nx, ndata]``), summed in np.longdouble and rounded to float64 -- with it the likelihood
    is ``-C/2`` of the C statistic, 0 for a perfect model.  Needs no device."""
    y = np.array(y, dtype=np.float64)
    e = np.ones_like(y) if e is None else np.array(e, dtype=np.float64)
    if e.shape != y.shape:
        raise ValueError("e and y differ in shape")
    masked = (e == 0) | np.isnan(e) | ~np.isfinite(y)
    bad = ~masked & ((e < 0) | (e == np.inf) | (y < 0))
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        if e[at] < 0 or e[at] == np.inf:
            raise ValueError("e%s = %r: exposures must be finite and >= 0 (0 or NaN masks a pixel)" % (list(at), float(e[at])))
        raise ValueError("y%s = %r: counts must be >= 0 (a non-finite one masks a pixel)" % (list(at), float(y[at])))
    y[masked] = 0.0
    e[masked] = 0.0
    good = y > 0                                              # (masked pixels hold 0 counts: not among these)
    n, ee = np.where(good, y, 1.0).astype(np.longdouble), np.where(good, e, 1.0).astype(np.longdouble)
    terms = np.where(good, n * (1 + np.log(ee) - np.log(n)), np.longdouble(0))
    return y, e, masked, terms.sum(axis=axis).astype(np.float64)


def background_pixels(y, e, b, g=None, axis=0):
    """What :class:`CountSpectra` uploads for source-region counts ``y`` with exposures ``e`` (``None``: ones) and
    background-region counts ``b`` with exposures ``g`` (``None``: ones; the area ratio included), all of one shape:
    ``(y, e, b, g, masked, offsets)``.  A pixel is MASKED -- all four values 0, a deleted channel to the likelihood -- where
    :func:`count_pixels` masks ``(y, e)`` or, by the same rule, ``(b, g)``: ``e`` or ``g`` 0 or NaN, ``y`` or ``b`` not
    finite.  On a pixel that is not masked a negative count and a negative or infinite exposure raise ValueError.
    ``offsets``: per spectrum ``Kw = sum n (1 + log e - log n) + sum b (1 + log g - log b)`` over its pixels with
    ``n > 0`` and ``b > 0``, in np.longdouble, rounded to float64: with it the likelihood is ``-W/2`` of the W statistic,
    0 where model plus fitted background reproduce both spectra.  Needs no device."""
    y, e, m1, _ = count_pixels(y, e, axis)
    b = np.array(b, dtype=np.float64)
    if b.shape != y.shape:
        raise ValueError("background and y differ in shape")
    b[m1] = 0.0                                               # (masked already: nothing of it is looked at)
    g = np.ones_like(b) if g is None else np.array(g, dtype=np.float64)
    if g.shape == b.shape:
        g[m1] = 0.0
    try:
        b, g, m2, _ = count_pixels(b, g, axis)
    except ValueError as err:
        raise ValueError("background: " + str(err).replace("e[", "g[", 1).replace("y[", "b[", 1).replace("e and y", "g and b"))
    masked = m1 | m2
    for a in (y, e, b, g):
        a[masked] = 0.0
    offsets = np.longdouble(0)
    for n, ee in ((y, e), (b, g)):
        good = n > 0                                          # (masked pixels hold 0 counts: not among these)
        nn, el = np.where(good, n, 1.0).astype(np.longdouble), np.where(good, ee, 1.0).astype(np.longdouble)
        offsets = offsets + np.where(good, nn * (1 + np.log(el) - np.log(nn)), np.longdouble(0)).sum(axis=axis)
    return y, e, b, g, masked, np.asarray(offsets).astype(np.float64)


class CountSpectra(_Spectra):
    """Photon counts scored against model curves the caller made (include/mdns.h Part 10): the Poisson likelihood
    ``L = sum_j (n_j log c_j - e_j c_j) + K``, the curve ``c >= 0`` the expected count RATE per unit ``exposure``
    (default 1) -- ``-C/2`` of the C statistic of X-ray fitting.  A pixel with ``exposure`` 0 or NaN, or a non-finite
    count, is masked (:func:`count_pixels`) and contributes nothing; ``n_masked`` [ndata] counts them per spectrum.  A
    curve value of 0 where counts were seen costs ``n log(DBL_MIN)``; a negative or NaN one makes the candidate's
    likelihood NaN for every spectrum.  A joint state on these spectra
    (:class:`massivedatans_amd.jointstate.CurveJointState`) scores its curve chunks the same way.

    With ``background`` -- the counts of a background region per spectrum, of ``y``'s shape, and ``background_exposure``
    (default 1; the area ratio included) -- ``y`` holds source PLUS background, the curve is the SOURCE rate, and the
    likelihood is the W statistic (include/mdns.h Part 11, mdns_curve_wstat_batch): an unknown background rate per pixel,
    profiled out of the joint Poisson likelihood of the two spectra.  A pixel masked on either side
    (:func:`background_pixels`) is masked; :meth:`background_fit` gives the fitted rates.  A curve value of 0 is then
    no penalty where the background can carry the counts."""

    continuum = 0

    def __init__(self, x, y, exposure=None, background=None, background_exposure=None, layout="channel_major"):
        channel_major = layout == "channel_major"
        axis = 0 if channel_major else 1
        if background is None and background_exposure is not None:
            raise ValueError("background_exposure needs background")
        self.has_background = background is not None
        if self.has_background:
            y, e, b, g, masked, kw = background_pixels(y, exposure, background, background_exposure, axis=axis)
            offsets = count_pixels(y, e, axis=axis)[3]           # (the C statistic's K of what is left: Part 10 on this handle)
        else:
            y, e, masked, offsets = count_pixels(y, exposure, axis=axis)
        super(CountSpectra, self).__init__(x, y, None, layout)
        self.n_masked = masked.sum(axis=0 if channel_major else 1)
        rows = None
        if exposure is not None or masked.any():              # one spectrum per row, as the handle keeps them
            rows = np.ascontiguousarray(e.T if channel_major else e)
        offsets = np.ascontiguousarray(offsets)
        rc = self._lib.mdns_spectra_set_counts(self._h, _lib.opt(rows), _lib.ptr(offsets))
        if rc != 0:
            self.close()
            _lib.check(rc, "mdns_spectra_set_counts")
        if self.has_background:
            b_rows = np.ascontiguousarray(b.T if channel_major else b)
            g_rows = np.ascontiguousarray(g.T if channel_major else g)
            kw = np.ascontiguousarray(kw)
            rc = self._lib.mdns_spectra_set_background(self._h, _lib.ptr(b_rows), _lib.ptr(g_rows), _lib.ptr(kw))
            if rc != 0:
                self.close()
                _lib.check(rc, "mdns_spectra_set_background")

    def loglike_batch_curves(self, curves, data_mask=None):
        """``curves[B, nx]`` -> ``L[B, mask.sum()]`` (mdns_curve_poisson_batch; with a background
        mdns_curve_wstat_batch)."""
        return self._curves_batch("mdns_curve_wstat_batch" if self.has_background else "mdns_curve_poisson_batch", curves, data_mask)

    def background_fit(self, curves, data_mask=None):
        """``curves[B, nx]`` -> ``f[B, M, nx]``: the background rate the W statistic fitted to every pixel of every pair,
        by the device functions its scoring kernel uses (mdns_curve_background_batch) -- ``curves + f`` is the "model +
        background" a caller plots against ``y / exposure``.  0 at a masked pixel."""
        if not self.has_background:
            raise ValueError("these spectra were made without a background")
        curves = np.atleast_2d(_lib.as_f64(curves))
        if curves.shape[1] != self.n_in:                      # (with a response: unfolded curves, folded on the device)
            raise ValueError("curves must be [B, %d]" % self.n_in)
        rows, M = _rows_from_mask(data_mask, self.ndata)
        B = len(curves)
        f = np.empty((B, M, self.nx))
        if B and M:
            _lib.check(self._lib.mdns_curve_background_batch(self._h, _lib.ptr(curves), B, _lib.opt(rows),
                                                             M, _lib.ptr(f)), "mdns_curve_background_batch")
        return f

    loglike_batch = loglike_batch_curves


class MuseSpectra(_Spectra):
    """Spectra with per-pixel variances scored against templates (cmuselike.c:45-64).  ``lines``:
    G rows ``(mu, a, sigma)`` of the template the device evaluates from parameters, ``ref`` the line
    whose ratio is 1 (:func:`massivedatans_amd.gen.muse_template`); None: the built-in three lines.
    ``continuum=P`` (1..4): every scoring on these spectra profiles a polynomial of P Legendre terms out per
    spectrum, together with the scale (:mod:`massivedatans_amd.continuum`; include/mdns.h Part 8)."""

    def __init__(self, x, y, v, layout="channel_major", lines=None, ref=1, continuum=0):
        from . import gen
        from .continuum import check_terms
        continuum = check_terms(continuum)
        if lines is not None:
            lines, ref = gen.check_lines(lines, ref)
        super(MuseSpectra, self).__init__(x, y, v, layout)
        self.lines, self.ref = lines, (ref if lines is not None else 1)
        if lines is not None:
            table = _lib.as_f64(lines)
            _lib.check(self._lib.mdns_spectra_set_lines(self._h, _lib.ptr(table), len(lines), ref), "mdns_spectra_set_lines")
        self.nparams = int(self._lib.mdns_spectra_nparams(self._h))
        self.continuum = 0
        if continuum:
            _lib.check(self._lib.mdns_spectra_set_continuum(self._h, continuum), "mdns_spectra_set_continuum")
            self.continuum = continuum

    def continuum_fit(self, ypred, data_mask=None):
        """``ypred[B, nx]`` -> ``(L[B, M], s[B, M], coef[B, M, P])``: the likelihood as ``loglike_batch`` gives it
        (the same kernel, the same bytes) with the fitted scale and continuum coefficients of every pair."""
        if not self.continuum:
            raise ValueError("these spectra were made without a continuum")
        ypred = np.atleast_2d(_lib.as_f64(ypred))
        if ypred.shape[1] != self.n_in:
            raise ValueError("templates must be [B, %d]" % self.n_in)
        rows, M = _rows_from_mask(data_mask, self.ndata)
        B = len(ypred)
        L, s, coef = np.empty((B, M)), np.empty((B, M)), np.empty((B, M, self.continuum))
        if B and M:
            _lib.check(self._lib.mdns_muse_continuum_fit_batch(self._h, _lib.ptr(ypred), B, _lib.opt(rows),
                                                               M, _lib.ptr(L), _lib.ptr(s), _lib.ptr(coef)),
                       "mdns_muse_continuum_fit_batch")
        return L, s, coef

    def loglike_batch(self, ypred, data_mask=None):
        """``ypred[B, nx]`` precomputed templates -> ``L[B, mask.sum()]`` (= -0.5 chi)."""
        ypred = np.atleast_2d(_lib.as_f64(ypred))
        if ypred.shape[1] != self.n_in:
            raise ValueError("templates must be [B, %d]" % self.n_in)
        return self._batch(self._lib.mdns_muse_loglike_batch, "mdns_muse_loglike_batch",
                           ypred, data_mask)

    def loglike_batch_lines(self, params, data_mask=None):
        """``params[B, 5]`` of the config-C5 three-line template -- ``[B, G + 2]`` of the line list
        these spectra were made with -- evaluated on the device."""
        params = np.atleast_2d(_lib.as_f64(params))
        if params.shape[1] != self.nparams:
            raise ValueError("params must be [B, %d]" % self.nparams)
        if self.lines is not None:
            return self._batch(self._lib.mdns_lines_loglike_batch, "mdns_lines_loglike_batch", params, data_mask)
        return self._batch(self._lib.mdns_muse3_loglike_batch, "mdns_muse3_loglike_batch",
                           params, data_mask)

    def templates(self, params):
        """``params[B, nparams]`` -> the templates ``[B, nx]`` as the device evaluates them."""
        params = np.atleast_2d(_lib.as_f64(params))
        if params.shape[1] != self.nparams:
            raise ValueError("params must be [B, %d]" % self.nparams)
        out = np.empty((len(params), self.nx))
        if out.size:
            _lib.check(self._lib.mdns_lines_template_batch(self._h, _lib.ptr(params), len(params), _lib.ptr(out)),
                       "mdns_lines_template_batch")
        return out

    def multi_loglikelihood(self, ypred, data_mask, jitter=None):
        """musefuse.py:534-535 given the template: masked likelihoods; ``jitter`` (e.g.
        ``numpy.random.normal``) reproduces the reference's N(0, 1e-5) tie-breaker and its RNG
        consumption."""
        if not np.any(ypred):
            # "give low probability to solutions with no stars" (musefuse.py:527-529): no kernel
            # call and -- unlike the regular path -- no random numbers drawn
            return np.ones(_rows_from_mask(data_mask, self.ndata)[1]) * -1e100
        L = self.loglike_batch(ypred, data_mask)[0]
        if jitter is not None:
            L = L + jitter(0, 1e-5, size=len(L))
        return L
