"""The MUSE-style problem of BASELINE.json configs[4]: one template fitted to N spectra with
per-pixel variances, amplitude marginalised per spectrum -- the likelihood of the reference's
``musefuse.py:520-535`` (``multi_loglikelihood_clike``: host template, then ``cmuselike.so``),
wired to the same sampler / integrator / constrainers as ``musefuse.py:607-675``.

What differs from the reference's script is the MODEL, by necessity: its stellar-population
template needs external grids and a FITS cube (musefuse.py:31-154,171-284) that are not part of
the repository; SURVEY.md 8(d) defines the stand-in used here and in BASELINE.json configs[4] --
three Gaussian emission lines on a flat continuum, 5 parameters
(:func:`massivedatans_amd.gen.muse_template`).  The line list of that family is the caller's to
choose: ``MuseProblem(..., lines=, ref=, prior=)``, 1 to 6 lines ``(mu, a, sigma)`` with common
redshift and width scale and free ratios against line ``ref`` -- G + 2 parameters, evaluated on the
device like the built-in three.  The LIKELIHOOD is the reference's, including
the ``N(0, 1e-5)`` tie-breaking noise it adds to every evaluation from the global random stream
(musefuse.py:535): with ``jitter=True`` (default) a run consumes the stream exactly as the
reference's loop would (tests/test_muse.py pins that against the reference's own sampler driven
with this problem); ``jitter=False`` drops the noise (kernel benchmarks).

    python -m massivedatans_amd.musefuse <cube.npz> <ndata>

``MUSE_LINES=<file.json>`` fits another line list: ``{"lines": [[mu, a, sigma], ...], "ref": k}``,
optionally with ``"prior": [[a, b], ...]`` (one pair per parameter, ``x = a * u + b``).
``MUSE_CONTINUUM=P`` (1..4) profiles a polynomial continuum of P Legendre terms out of every spectrum,
together with its scale (:mod:`massivedatans_amd.continuum`); unset or 0: none.
"""
import json
import os
import sys
import time

import numpy

from . import cachedconstrainer, gen
from .multi_nested_integrator import multi_nested_integrator

paramnames = ['log_amp', 'z', 'log_width', 'ratio1', 'ratio3']
nparams = len(paramnames)
#: unit cube -> parameter, per dimension: x = a * u + b
PRIOR = ((2.0, -1.0), (0.02, 0.0), (1.0, -0.5), (1.8, 0.2), (1.8, 0.2))
#: prior of the ratio of a line a caller adds
RATIO_PRIOR = (1.8, 0.2)
JITTER_SIGMA = 1e-5                       # musefuse.py:535


def _transform(cube, prior):
    cube = cube.copy()
    for k, (a, b) in enumerate(prior):
        cube[k] = cube[k] * a + b if b != 0.0 else cube[k] * a
    return cube


def _transform_batch(cubes, prior):
    cubes = numpy.asarray(cubes, dtype=float)
    out = numpy.empty_like(cubes)
    for k, (a, b) in enumerate(prior):
        out[:, k] = cubes[:, k] * a + b if b != 0.0 else cubes[:, k] * a
    return out


def priortransform(cube):
    return _transform(cube, PRIOR)


def priortransform_batch(cubes):
    return _transform_batch(cubes, PRIOR)


def lines_paramnames(lines, ref):
    """(log_amp, z, log_width, ratio of every line but ``ref``, numbered from 1 in list order)"""
    return ['log_amp', 'z', 'log_width'] + ['ratio%d' % (g + 1) for g in range(len(lines)) if g != ref]


def lines_prior(lines, prior=None):
    """``(a, b)`` per parameter of a line list: the built-in model's for amplitude, redshift and
    width scale, RATIO_PRIOR for every ratio; ``prior`` (a pair or None per parameter) overrides."""
    n = len(lines) + 2
    out = list(PRIOR[:3]) + [RATIO_PRIOR] * (n - 3)
    if prior is not None:
        prior = list(prior)
        if len(prior) != n:
            raise ValueError("prior needs one (a, b) pair per parameter: %d, not %d" % (n, len(prior)))
        for k, ab in enumerate(prior):
            if ab is None:
                continue
            try:
                a, b = (float(t) for t in ab)
            except (TypeError, ValueError):
                raise ValueError("prior[%d] must be a pair (a, b), got %r" % (k, ab))
            if not (numpy.isfinite(a) and numpy.isfinite(b)):
                raise ValueError("prior[%d] = (%r, %r) is not finite" % (k, a, b))
            out[k] = (a, b)
    return tuple(out)


def read_lines(path):
    """A ``MUSE_LINES`` file -> ``(lines, ref, prior or None)``; ValueError says what is wrong with it."""
    try:
        with open(path) as f:
            spec = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError("cannot read a line list from %s: %s" % (path, e))
    if not isinstance(spec, dict) or not isinstance(spec.get("lines"), list):
        raise ValueError('%s: expected {"lines": [[mu, a, sigma], ...], "ref": k}' % path)
    unknown = sorted(set(spec) - {"lines", "ref", "prior"})
    if unknown:
        raise ValueError("%s: unknown keys %s" % (path, ", ".join(unknown)))
    if "ref" not in spec:
        raise ValueError('%s: "ref" (the line whose ratio is 1) is missing' % path)
    try:
        lines, ref = gen.check_lines(spec["lines"], spec["ref"])
        prior = spec.get("prior")
        if prior is not None:
            if not isinstance(prior, list):
                raise ValueError('"prior" must be a list of [a, b] pairs')
            prior = lines_prior(lines, prior)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e))
    return lines, ref, prior


def write_lines(path, lines, ref, prior=None):
    spec = {"lines": [list(row) for row in lines], "ref": int(ref)}
    if prior is not None:
        spec["prior"] = [list(ab) for ab in prior]
    with open(path, "w") as f:
        json.dump(spec, f)


def kernel_params(xs):
    """The device template takes the physical parameters as they are."""
    return numpy.array(xs, dtype=float)


def native_prior(jitter, prior=PRIOR):
    from . import constrainer
    p = constrainer.Prior()
    p.ndim, p.nparams = len(prior), len(prior)
    for k, (a, b) in enumerate(prior):
        p.a[k], p.b[k], p.pow10[k], p.kernel_pow10[k] = a, b, 0, 0
    p.jitter_sigma = JITTER_SIGMA if jitter else 0.0
    return p


class MuseProblem(object):
    """``x`` f64[nx], ``y`` / ``v`` f64[nx, ndata] (the reference's layout, cmuselike.c:54).
    ``backend``: any object with ``loglike_batch(ypred[B, nx], data_mask) -> L[B, M]`` and
    ``loglike_batch_lines(params[B, 5], data_mask)`` (tests inject the CPU oracle there); by
    default :class:`massivedatans_amd.like.MuseSpectra` on the GPU.

    ``lines`` (G rows ``(mu, a, sigma)``, 1 <= G <= 6) and ``ref`` choose the line list, ``prior``
    (one ``(a, b)`` pair or None per parameter) overrides the default prior; parameter names, count
    and prior transforms follow.  A GPU backend evaluates the list on the device (it must have been
    made with the same list); of any other backend only ``loglike_batch`` is used, over
    :func:`massivedatans_amd.gen.muse_template` in numpy.

    ``continuum=P`` (1..4): a polynomial of P Legendre terms per spectrum is profiled out with the scale
    (:mod:`massivedatans_amd.continuum`).  A backend must have been made with the same ``continuum``
    (:class:`massivedatans_amd.continuum.ContinuumScorer` is the CPU one); sharded backends have none."""

    paramnames = paramnames
    nparams = nparams
    PRIOR = PRIOR
    priortransform = staticmethod(priortransform)
    priortransform_batch = staticmethod(priortransform_batch)

    def __init__(self, x, y, v, backend=None, jitter=True, lines=None, ref=1, prior=None, continuum=0):
        from .continuum import check_terms
        self.continuum = check_terms(continuum)
        self.x = numpy.ascontiguousarray(x, dtype=float)
        self.y = numpy.ascontiguousarray(y, dtype=float)
        self.v = numpy.ascontiguousarray(v, dtype=float)
        self.nx, self.ndata = self.y.shape
        self.jitter = bool(jitter)
        self.lines, self.ref = None, 1
        if lines is not None:
            self.lines, self.ref = gen.check_lines(lines, ref)
            self.paramnames = lines_paramnames(self.lines, self.ref)
            self.nparams = len(self.paramnames)
        if lines is not None or prior is not None:
            table = lines_prior(self.lines if lines is not None else gen.MUSE_LINES, prior)
            self.PRIOR = table
            self.priortransform = lambda cube: _transform(cube, table)
            self.priortransform_batch = lambda cubes: _transform_batch(cubes, table)
        if backend is None:
            from .like import MuseSpectra
            backend = MuseSpectra(self.x, self.y, self.v, lines=self.lines, ref=self.ref, continuum=self.continuum)
        elif hasattr(backend, "lines") and (backend.lines, backend.ref) != (self.lines, self.ref):
            raise ValueError("the backend was made with another line list than the problem")
        elif getattr(backend, "continuum", 0) != self.continuum:
            from . import parallel
            if isinstance(backend, parallel.ShardedMuse):
                raise ValueError("continuum = %d: sharded runs do not fit a per-spectrum continuum" % self.continuum)
            raise ValueError("the backend was made with continuum = %r, the problem with %d"
                             % (getattr(backend, "continuum", 0), self.continuum))
        self.backend = backend
        self.ncalls = 0
        self.nevals = 0

    def model(self, params):
        if self.lines is None:
            return gen.muse_template(self.x, params)
        return gen.muse_template(self.x, params, self.lines, self.ref)

    def multi_loglikelihood(self, params, data_mask):
        """musefuse.py:520-535: template on the host, the C likelihood, the noise."""
        ypred = self.model(params)
        if not numpy.any(ypred):
            return numpy.ones(int(numpy.count_nonzero(data_mask))) * -1e100        # musefuse.py:527-529
        L = self.backend.loglike_batch(ypred[None, :], data_mask)[0]
        self.ncalls += 1
        self.nevals += len(L)
        if self.jitter:
            L = L + numpy.random.normal(0, JITTER_SIGMA, size=len(L))
        return L

    multi_loglikelihood_batch = None          # (every evaluation draws its noise: one candidate at a time)

    def native_prior(self):
        return native_prior(self.jitter, self.PRIOR)

    def joint_state(self, nlive_points):
        from . import jointstate, parallel
        from .like import MuseSpectra

        def build(scorer, ndata):
            if isinstance(scorer, MuseSpectra):
                return jointstate.MuseJointState(scorer, nlive_points)
            if self.lines is not None:
                return jointstate.HostJointState(TemplateScorer(scorer, self.x, self.lines, self.ref), nlive_points, ndata,
                                                 kernel_params, nparams=self.nparams)
            return jointstate.HostJointState(_LinesScorer(scorer), nlive_points, ndata, kernel_params, nparams=nparams)

        if isinstance(self.backend, parallel.ShardedMuse):
            # one process per GPU: every rank keeps the state of ITS block of data sets
            b = self.backend
            js = parallel.ShardedJointState(build(b.local, b.hi - b.lo), self.ndata, b.lo, b.hi)
        else:
            js = build(self.backend, self.ndata)
        js.jitter_sigma = JITTER_SIGMA if self.jitter else 0.0
        return js


class _LinesScorer(object):
    """``loglike_batch(params[B, 5], mask)`` over a backend that scores line parameters."""

    def __init__(self, backend):
        self.backend = backend

    def loglike_batch(self, params, data_mask=None):
        return self.backend.loglike_batch_lines(params, data_mask)


class TemplateScorer(object):
    """``loglike_batch(params[B, G + 2], mask)`` of a line list over a backend that scores TEMPLATES
    (``backend.loglike_batch(ypred[B, nx], mask)``): the templates in numpy
    (:func:`massivedatans_amd.gen.muse_template`) -- the host statement of what the device does with
    a line list."""

    def __init__(self, backend, x, lines, ref):
        self.backend = backend
        self.x = numpy.ascontiguousarray(x, dtype=float)
        self.lines, self.ref = gen.check_lines(lines, ref)

    def templates(self, params):
        params = numpy.atleast_2d(numpy.asarray(params, dtype=float))
        if params.shape[1] != len(self.lines) + 2:
            raise ValueError("params must be [B, %d]" % (len(self.lines) + 2))
        return numpy.array([gen.muse_template(self.x, p, self.lines, self.ref) for p in params]).reshape(len(params), len(self.x))

    def loglike_batch(self, params, data_mask=None):
        return self.backend.loglike_batch(self.templates(params), data_mask)


def run(x, y, v, nlive_points=400, nsuperset_draws=10, use_graph=True, max_samples=0, min_samples=0,
        tolerance=0.5, seed=1, backend=None, jitter=True, fused=True, native=None, lines=None, ref=1, prior=None,
        continuum=0):
    """The whole analysis (musefuse.py:607-648); returns ``(results, sampler, problem, duration)``."""
    from .sample import build_sampler, integrate
    problem = MuseProblem(x, y, v, backend=backend, jitter=jitter, lines=lines, ref=ref, prior=prior, continuum=continuum)
    start = time.time()
    sampler = build_sampler(problem, nlive_points, nsuperset_draws, use_graph, seed, batched=False, fused=fused, native=native)
    results = integrate(sampler, tolerance, min_samples, max_samples)
    if sampler.native is not None:
        sampler.native.sync_gauss_to_numpy()
    return results, sampler, problem, time.time() - start


def distributed_backend(x, y, v, lines=None, ref=1, continuum=0):
    """One process per GPU (torchrun): this rank's block of spectra and variances on its GPU behind
    :class:`parallel.ShardedMuse`; None in a single process (see sample.distributed_backend).  Sharded runs
    fit no per-spectrum continuum: ValueError."""
    from . import sample
    from .parallel import ShardedMuse
    if sample.distributed_setup() is None:
        return None
    if continuum:
        raise ValueError("continuum = %r: sharded runs do not fit a per-spectrum continuum (run in one process)" % (continuum,))
    from .like import MuseSpectra
    return ShardedMuse(x, y, v, lambda xs, ys, vs, **kw: MuseSpectra(xs, ys, vs, **kw), lines=lines, ref=ref)


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 3:
        sys.exit("usage: python -m massivedatans_amd.musefuse <cube.npz with x, y, v> <ndata>")
    ndata = int(argv[2])
    lines, ref, prior = None, 1, None
    if os.environ.get('MUSE_LINES'):
        try:
            lines, ref, prior = read_lines(os.environ['MUSE_LINES'])
        except ValueError as e:
            sys.exit("MUSE_LINES: %s" % e)
    continuum = 0
    if os.environ.get('MUSE_CONTINUUM'):
        from .continuum import MAX_TERMS
        try:
            continuum = int(os.environ['MUSE_CONTINUUM'])
            if not 0 <= continuum <= MAX_TERMS:
                raise ValueError
        except ValueError:
            sys.exit("MUSE_CONTINUUM: %r is not an integer in 0..%d (terms of the per-spectrum polynomial)"
                     % (os.environ['MUSE_CONTINUUM'], MAX_TERMS))
    data = gen.load(argv[1], ndata)
    nlive_points = int(os.environ.get('NLIVE_POINTS', '400'))
    results, sampler, problem, duration = run(
        data['x'], data['y'], data['v'], nlive_points=nlive_points, lines=lines, ref=ref, prior=prior, continuum=continuum,
        backend=distributed_backend(data['x'], data['y'], data['v'], lines, ref, continuum),
        nsuperset_draws=int(os.environ.get('SUPERSET_DRAWS', '10')), use_graph=os.environ.get('USE_GRAPH', '1') == '1',
        max_samples=int(os.environ.get('MAXSAMPLES', 100000)), min_samples=int(os.environ.get('MINSAMPLES', 0)))
    from .sample import write_outputs
    prefix = '%s_full_.out_%d' % (argv[1], ndata)
    first = write_outputs(prefix, results, sampler, duration, ndata)
    from .postprocess import run_posterior_outputs
    run_posterior_outputs(prefix, results)                            # MDNS_POSTERIOR=N; unset: nothing
    if not first:
        return
    print('logZ = %.1f +- %.1f' % (results['logZ'][0], results['logZerr'][0]))
    print('ndraws:', sampler.ndraws, 'niter:', len(results['weights']), 'in %.1f s' % duration)


if __name__ == '__main__':
    main()
