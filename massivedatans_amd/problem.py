"""A problem definition the caller writes: any model that makes one curve per candidate.

The reference's first instruction to its user is "Set your problem definition (parameters, model,
likelihood) in sample.py": a host-side function predicts one model curve per candidate and the data
comparison runs that curve over all spectra (sample.py:60-71; musefuse.py:222-284,520-535 is the same
pattern with a stellar-population grid).  :class:`CurveProblem` is that pattern with the whole
constrained draw on the device: the caller's ``model`` makes the curves of a chunk of candidates --
in numpy, or in torch on the GPU --, and scoring, thresholds, accept test and commit happen in
:class:`massivedatans_amd.jointstate.CurveJointState`.

    import numpy
    from massivedatans_amd import problem, sample

    def model(xs):                       # xs[B, 4] -> curves[B, nx]: a broad and a narrow line
        A, mu, broad, narrow = (xs[:, k, None] for k in range(4))
        return A * (numpy.exp(-0.5 * ((mu - x) / broad) ** 2) + numpy.exp(-0.5 * ((mu - x) / narrow) ** 2))

    def priortransform_batch(us):        # us[B, 4] in the unit cube -> xs[B, 4]
        return numpy.column_stack((10 ** (2 * us[:, 0] - 2), 400 + 400 * us[:, 1], 10 + 90 * us[:, 2], 1 + 9 * us[:, 3]))

    p = problem.CurveProblem(x, y, model, priortransform_batch, ndim=4, noise_level=0.01)
    results, sampler, p, seconds = sample.run_model(p, nlive_points=400)
"""
import numpy

MAX_DIM = 16                                 # include/mdns.h MDNS_MAX_DIM


def default_backend(x, y, noise_level, v=None, continuum=0, marginalise_scale=True, poisson=False, exposure=None,
                    background=None, background_exposure=None, response=None):
    """The spectra on the GPU: fixed noise, or -- with variances ``v`` -- the scale-marginalised likelihood
    (``continuum``: like.MuseSpectra), or -- ``marginalise_scale=False`` -- the fixed-scale one (like.WeightedSpectra), or
    -- ``poisson=True``, ``y`` holding counts -- the Poisson one (``exposure``: like.CountSpectra), with ``background``
    (and ``background_exposure``) the W statistic.  ``response`` (a :class:`massivedatans_amd.response.Response`) is
    attached: the spectra then take curves of ``response.n_in`` bins and fold them on the device."""
    from .like import CountSpectra, GaussLineSpectra, MuseSpectra, WeightedSpectra
    if poisson:
        spectra = CountSpectra(x, y, exposure, background, background_exposure)
    elif v is None:
        spectra = GaussLineSpectra(x, y, noise_level=noise_level)
    elif not marginalise_scale:
        spectra = WeightedSpectra(x, y, v)
    else:
        spectra = MuseSpectra(x, y, v, continuum=continuum)
    if response is not None:
        try:
            spectra.set_response(response)
        except Exception:
            spectra.close()
            raise
    return spectra


def host_curves(curves):
    """What a model returned as a float64 numpy array (a device tensor comes over)."""
    if hasattr(curves, "detach"):
        curves = curves.detach().cpu().numpy()
    return numpy.ascontiguousarray(curves, dtype=float)


class _ModelScorer(object):
    """``loglike_batch(xs[B, ndim], mask)`` = the backend's score of the model's curves."""

    def __init__(self, score, model):
        self.score, self.model = score, model

    def loglike_batch(self, xs, data_mask=None):
        return self.score(host_curves(self.model(numpy.asarray(xs, dtype=float))), data_mask)


class CurveProblem(object):
    """``x`` f64[nx], ``y`` (and ``v``) f64[nx, ndata] in the reference's layout.  ``model(xs[B, ndim]) ->
    curves[B, nx]`` and ``priortransform_batch(us[B, ndim]) -> xs[B, ndim]`` are the caller's.  Four
    likelihoods:

    * without ``v``: ``-0.5 sum_j ((curve_j - y_j) / noise_level)**2`` (sample.py:64-71), one noise level for every
      pixel;
    * with per-pixel variances ``v``: the scale-marginalised one of cmuselike.c:45-64 -- a free amplitude ``s`` per
      spectrum is fitted, ``-0.5 sum_j (y_j - s curve_j)**2 / v_j`` (``noise_level`` is not used); with
      ``continuum=P`` (1..4; needs ``v``) a polynomial of P Legendre terms is profiled out per spectrum as well
      (:mod:`massivedatans_amd.continuum`).  The amplitude of the model drops out: do not make it a parameter;
    * with ``v`` and ``marginalise_scale=False``: ``-0.5 sum_j (curve_j - y_j)**2 / v_j`` at FIXED scale, for a
      model whose amplitude is a parameter.  A pixel with ``v = inf`` (or NaN, or a non-finite ``y``) is ignored
      (:class:`massivedatans_amd.like.WeightedSpectra`).  Needs ``v``, excludes ``continuum``;
    * with ``poisson=True``: ``y`` holds photon COUNTS, the curve is the expected count rate per unit ``exposure``
      (f64[nx, ndata], default 1) and the likelihood the Poisson one, ``sum_j (y_j log curve_j - exposure_j curve_j)``
      plus a constant per spectrum that makes it ``-C/2`` of the C statistic.  The curve must be ``>= 0``: 0 where counts
      were seen costs about ``-708`` per count, a negative or NaN value makes the candidate NaN for every spectrum (it is
      then never accepted).  A pixel with ``exposure`` 0 (or NaN, or a non-finite count) is ignored
      (:class:`massivedatans_amd.like.CountSpectra`).  Excludes ``v``, ``continuum`` and ``marginalise_scale=False``;
      ``noise_level`` is not used;
    * with ``poisson=True`` and ``background`` (f64[nx, ndata], the counts of a background region per spectrum;
      ``background_exposure`` the same shape, default 1, the area ratio included): ``y`` holds source plus background,
      the curve is the SOURCE rate, and the likelihood is the W statistic -- an unknown background rate per pixel,
      profiled out in closed form of the joint Poisson likelihood of the two spectra (include/mdns.h Part 11).  A pixel
      masked on either side is ignored; ``backend.background_fit`` gives the fitted rates.

    ``model`` may also be a :class:`massivedatans_amd.tablemodel.TableModel` (``ndim`` must be its ``ndim``), with every
    likelihood above: the device then interpolates the table per candidate and scores the curves where they lie --
    draws and the initial points hand over parameters (``mdns_backend_draw_table``, ``mdns_joint_init_table``) and no
    curve is made in Python; ``multi_loglikelihood[_batch]`` fetch the device's curves and score them like any other.
    Over a ``backend`` that is not on the device the model is ``TableModel.statement``.  A
    :class:`massivedatans_amd.summodel.SumModel` -- a sum of tables, power laws and Gaussian lines with an optional common
    attenuation (include/mdns.h Part 14) -- is taken in the same way (``mdns_backend_draw_sum``, ``mdns_joint_init_sum``;
    elsewhere ``SumModel.statement``).

    ``response`` (a :class:`massivedatans_amd.response.Response` of ``nx`` channels; works with every likelihood above):
    the instrument response between the model and the data.  ``model`` then returns ``[B, response.n_in]``, on the
    response's model bins, and every curve is folded onto the channels on the device before it is scored (include/mdns.h
    Part 13); a ``TableModel`` is evaluated on ``response.x_in``; ``multi_loglikelihood[_batch]`` and
    ``backend.background_fit`` take unfolded curves.  Over a ``backend`` that is not on the device the model becomes
    ``response.statement(model(xs))``.  One response serves all spectra of the run (a per-spectrum effective area goes
    into ``exposure``); sharded runs and the chained first batch do not take one.

    ``jitter_sigma > 0`` adds ``N(0, jitter_sigma)`` to every likelihood evaluation from the global random
    stream, as musefuse.py:535 does.  ``backend``: any object with ``loglike_batch(curves[B, nx], mask) ->
    L[B, M]`` (tests put a numpy scorer there; the state is then the numpy one); by default the spectra go
    to the GPU.

    Gives ``sample.build_sampler`` what it reads of a problem."""

    def __init__(self, x, y, model, priortransform_batch, ndim, noise_level=0.01, v=None, jitter_sigma=0.0, backend=None,
                 continuum=0, marginalise_scale=True, poisson=False, exposure=None, background=None, background_exposure=None,
                 response=None):
        from .continuum import check_terms
        from .response import Response
        self.continuum = check_terms(continuum)
        self.marginalise_scale = bool(marginalise_scale)
        self.poisson = bool(poisson)
        if self.poisson and v is not None:
            raise ValueError("poisson = True excludes the variances v (the noise of counts is Poisson, not Gaussian)")
        if self.poisson and self.continuum:
            raise ValueError("poisson = True excludes continuum = %d (it belongs to the scale-marginalised likelihood)" % self.continuum)
        if self.poisson and not self.marginalise_scale:
            raise ValueError("poisson = True excludes marginalise_scale = False (that is the Gaussian likelihood with variances)")
        if exposure is not None and not self.poisson:
            raise ValueError("exposure needs poisson = True (the Gaussian likelihoods have no exposure)")
        if background is not None and not self.poisson:
            raise ValueError("background needs poisson = True (the W statistic is a likelihood of counts)")
        if background_exposure is not None and background is None:
            raise ValueError("background_exposure needs background")
        if self.continuum and v is None:
            raise ValueError("continuum = %d needs the variances v (the scale-marginalised likelihood)" % self.continuum)
        if not self.marginalise_scale and v is None:
            raise ValueError("marginalise_scale = False needs the variances v (without them the likelihood is the fixed-noise one)")
        if not self.marginalise_scale and self.continuum:
            raise ValueError("marginalise_scale = False excludes continuum = %d (the continuum is profiled out together with the scale)"
                             % self.continuum)
        self.x = numpy.ascontiguousarray(x, dtype=float)
        self.y = numpy.ascontiguousarray(y, dtype=float)
        self.v = None if v is None else numpy.ascontiguousarray(v, dtype=float)
        self.exposure = None if exposure is None else numpy.ascontiguousarray(exposure, dtype=float)
        self.background = None if background is None else numpy.ascontiguousarray(background, dtype=float)
        self.background_exposure = None if background_exposure is None else numpy.ascontiguousarray(background_exposure, dtype=float)
        for name in ("background", "background_exposure"):
            a = getattr(self, name)
            if a is not None and a.shape != self.y.shape:
                raise ValueError("%s has shape %s, y has %s" % (name, a.shape, self.y.shape))
        self.nx, self.ndata = self.y.shape
        if response is not None and not isinstance(response, Response):
            raise ValueError("response must be a massivedatans_amd.response.Response, got %r" % type(response).__name__)
        if response is not None and response.nx != self.nx:
            raise ValueError("the response folds onto %d channels, y has %d" % (response.nx, self.nx))
        self.response = response
        if not 1 <= int(ndim) <= MAX_DIM:
            raise ValueError("ndim = %r: 1 to %d parameters" % (ndim, MAX_DIM))
        self.nparams = int(ndim)
        from .summodel import SumModel
        from .tablemodel import TableModel
        # (a sum model, massivedatans_amd.summodel, is treated exactly like a table model: bound to the device, or its statement)
        table_model = model if isinstance(model, (TableModel, SumModel)) else None
        kind = "sum" if isinstance(model, SumModel) else "table"
        if table_model is not None and table_model.ndim != self.nparams:
            raise ValueError("ndim = %d, the %s model takes %d parameters" % (self.nparams, kind, table_model.ndim))
        if table_model is not None and response is not None and response.x_in is None:
            raise ValueError("a %s model under a response is evaluated on the response's model bins: the response needs x_in" % kind)
        model_x = self.x if response is None else response.x_in     # the abscissa a table model is bound to
        self.table = None                            # a table model on the device (tablemodel.DeviceTable, summodel.DeviceSum)
        self.model = model
        self.priortransform_batch = priortransform_batch
        self.noise_level = float(noise_level)
        self.jitter_sigma = float(jitter_sigma)
        if backend is None:
            kw = dict(continuum=self.continuum) if self.continuum else {}
            if not self.marginalise_scale:
                kw["marginalise_scale"] = False
            if self.poisson:
                kw["poisson"] = True
                if self.exposure is not None:
                    kw["exposure"] = self.exposure
                if self.background is not None:
                    kw["background"] = self.background
                if self.background_exposure is not None:
                    kw["background_exposure"] = self.background_exposure
            if response is not None:
                kw["response"] = response
            backend = default_backend(self.x, self.y, self.noise_level, self.v, **kw)
        self.backend = backend
        if response is not None and self._on_device():
            attached = getattr(backend, "response", None)
            if attached is None or attached.response is not response:
                raise ValueError("the backend was made without this response (default_backend(..., response=) attaches it)")
        if getattr(backend, "continuum", 0) != self.continuum:
            raise ValueError("the backend was made with continuum = %r, the problem with %d"
                             % (getattr(backend, "continuum", 0), self.continuum))
        if table_model is not None:
            # on the device the joint state hands parameters to the table (no curves are made in Python); what scores
            # outside a draw fetches the device's curves.  Over any other backend the model is its numpy statement
            if self._on_device():
                self.table = table_model.bind(model_x)
                self.model = self.table.curves
            else:
                self.model = lambda xs, _tm=table_model, _x=model_x: _tm.statement(_x, xs)
        if response is not None and not self._on_device():
            # (on the device the spectra fold; over any other backend the model does, by the numpy statement)
            self.model = lambda xs, _m=self.model, _r=response: _r.statement(host_curves(_m(xs)))
        if jitter_sigma > 0:
            self.multi_loglikelihood_batch = None         # (every evaluation draws its noise: one candidate at a time)
        self.ncalls = 0
        self.nevals = 0

    def priortransform(self, cube):
        return numpy.asarray(self.priortransform_batch(numpy.asarray(cube, dtype=float)[None, :]), dtype=float)[0]

    def _on_device(self):
        from .like import _Spectra
        return isinstance(self.backend, _Spectra)

    def _score(self, curves, data_mask):
        if hasattr(self.backend, "loglike_batch_curves"):
            return self.backend.loglike_batch_curves(curves, data_mask)
        return self.backend.loglike_batch(curves, data_mask)

    def multi_loglikelihood(self, params, data_mask):
        L = self._score(host_curves(self.model(numpy.asarray(params, dtype=float)[None, :])), data_mask)[0]
        self.ncalls += 1
        self.nevals += len(L)
        if self.jitter_sigma > 0:
            L = L + numpy.random.normal(0, self.jitter_sigma, size=len(L))
        return L

    def multi_loglikelihood_batch(self, params, data_mask):
        L = self._score(host_curves(self.model(numpy.asarray(params, dtype=float))), data_mask)
        self.ncalls += 1
        self.nevals += L.size
        return L

    def native_prior(self):
        """The prior transform stays in Python, the kernel parameters are the physical ones (the model takes them)."""
        from . import constrainer
        p = constrainer.custom_prior(self.nparams, self.nparams, self.priortransform_batch, lambda xs: xs)
        p.jitter_sigma = self.jitter_sigma
        return p

    def joint_state(self, nlive_points):
        from . import jointstate
        if self._on_device():
            js = jointstate.CurveJointState(self.backend, nlive_points, self.model, ndim=self.nparams, table=self.table)
        else:
            js = jointstate.HostJointState(_ModelScorer(self._score, self.model), nlive_points, self.ndata,
                                           lambda xs: xs, nparams=self.nparams)
        js.jitter_sigma = self.jitter_sigma
        return js


__all__ = ['CurveProblem', 'default_backend']
