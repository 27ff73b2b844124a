"""Per-data-set posterior summaries and equal-weight draws of a finished run, on the GPU
(``include/mdns.h`` Part 7, ``csrc/mdns_posterior.hip``).

The counterpart of the reference's per-spectrum post-processing loop (musefuse_postprocess.py:112-140,
checkoutput.py:27-44): for every data set ``d`` the rows ``F`` where ``lw = w + L`` is finite, the weights
``p = exp(lw[F] - max) / sum``, the weighted mean, standard deviation and quantiles of every parameter,
the Kish effective sample size, and draws equal to
``Generator(Philox(key=[seed, d])).choice(F, n, p=p)``.  There is no CPU path: without a device
:class:`Posterior` raises :class:`~massivedatans_amd._lib.MdnsError`.
"""
import ctypes as C

import numpy as np

from . import _lib

#: device milliseconds reported by :meth:`Posterior.timings`
PHASES = ("moments", "std", "quantiles", "resample")


class Posterior(object):
    """``w``, ``L`` ``[nsamp, ndata]`` and ``x`` ``[nsamp, ndata, ndim]`` (as ``save_results`` writes them),
    uploaded once to the device; :meth:`summary` and :meth:`resample` share the upload."""

    def __init__(self, w, L, x):
        w, L, x = _lib.as_f64(w), _lib.as_f64(L), _lib.as_f64(x)
        if w.ndim != 2 or L.shape != w.shape or x.ndim != 3 or x.shape[:2] != w.shape:
            raise ValueError("want w, L [nsamp, ndata] and x [nsamp, ndata, ndim]; got %s, %s, %s"
                             % (w.shape, L.shape, x.shape))
        self.nsamp, self.ndata, self.ndim = x.shape
        self._h = None
        lib = _lib.require_device()
        h = lib.mdns_posterior_create(_lib.ptr(w), _lib.ptr(L), _lib.ptr(x), self.nsamp, self.ndata, self.ndim)
        if not h:
            raise _lib.MdnsError("mdns_posterior_create failed: %s" % _lib.last_error())
        self._h = C.c_void_p(h)

    def close(self):
        if self._h is not None:
            _lib.load().mdns_posterior_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def summary(self, quantiles=(0.16, 0.5, 0.84)):
        """dict of ``nfinite``, ``log_norm``, ``ess``, ``imaxL`` ``[ndata]``, ``mean``, ``std``
        ``[ndata, ndim]``, ``quant`` ``[ndata, ndim, nq]`` and ``q``."""
        q = _lib.as_f64(quantiles).reshape(-1)
        nd, k = self.ndata, self.ndim
        out = dict(nfinite=np.empty(nd, np.int32), log_norm=np.empty(nd), ess=np.empty(nd),
                   mean=np.empty((nd, k)), std=np.empty((nd, k)), quant=np.empty((nd, k, len(q))),
                   imaxL=np.empty(nd, np.int32))
        rc = _lib.load().mdns_posterior_summary(
            self._h, _lib.ptr(q), len(q), _lib.ptr(out['nfinite']), _lib.ptr(out['log_norm']), _lib.ptr(out['ess']),
            _lib.ptr(out['mean']), _lib.ptr(out['std']), _lib.ptr(out['quant']) if len(q) else None,
            _lib.ptr(out['imaxL']))
        _lib.check(rc, "mdns_posterior_summary")
        out['q'] = q
        return out

    def resample(self, n, seed=1, gather=False, first_column=0):
        """``index`` int32 ``[ndata, n]`` (rows of the run; -1 for a data set without finite weights), and
        with ``gather`` also the drawn parameters ``[ndata, n, ndim]``: ``(index, xdraws)``.  Data set ``d``
        draws from ``Philox(key=[seed, first_column + d])``."""
        n = int(n)
        index = np.empty((self.ndata, n), np.int32)
        xdraws = np.empty((self.ndata, n, self.ndim)) if gather else None
        rc = _lib.load().mdns_posterior_resample(self._h, C.c_ulonglong(int(seed)), C.c_longlong(int(first_column)), n,
                                                 _lib.ptr(index), _lib.ptr(xdraws) if gather else None)
        _lib.check(rc, "mdns_posterior_resample")
        return (index, xdraws) if gather else index

    def timings(self):
        """Device milliseconds of the last calls, by phase (``PHASES``)."""
        ms = np.zeros(len(PHASES))
        _lib.check(_lib.load().mdns_posterior_timings(self._h, _lib.ptr(ms)), "mdns_posterior_timings")
        return dict(zip(PHASES, ms.tolist()))


def weights_arrays(weights):
    """``w``, ``L`` ``[nsamp, ndata]`` and ``x`` ``[nsamp, ndata, ndim]`` of ``results['weights']``
    (the arrays ``save_results`` writes)."""
    _, x, L, w, _ = list(zip(*weights))
    return np.array(w), np.array(L), np.array(x)


def summarize_results(results, quantiles=(0.16, 0.5, 0.84), resample=0, seed=1):
    """Summary (and, with ``resample`` > 0, that many draws per data set) of ``multi_nested_integrator``'s
    result dict.  A sharded rank's results carry ``columns`` = (lo, hi) and the weights of those data sets
    only; ``logZ`` / ``logZerr`` are then cut to the same columns.  Returns the dict that
    ``postprocess`` writes."""
    w, L, x = weights_arrays(results['weights'])
    lo, hi = results.get('columns', (0, w.shape[1]))
    with Posterior(w, L, x) as post:
        out = post.summary(quantiles)
        if resample:
            out['index'] = post.resample(resample, seed=seed, first_column=lo)
            out['seed'] = np.uint64(seed)
    logZ, logZerr = np.atleast_1d(results['logZ']), np.atleast_1d(results['logZerr'])
    if len(logZ) != hi - lo:
        logZ, logZerr = logZ[lo:hi], logZerr[lo:hi]
    out.update(logZ=logZ, logZerr=logZerr, columns=np.array([lo, hi]))
    return out
