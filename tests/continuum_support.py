"""Case builders and the extended-precision statement for the continuum tests (tests/test_continuum_host.py,
tests/test_continuum.py).

The reference of every comparison is ``massivedatans_amd.continuum.loglike_statement(..., dtype=np.longdouble)``:
the definition of the likelihood, with ``G`` factored and solved in longdouble.  The tolerance for ``L`` against it
is the project's K2 figure, 1e-11 relative (tests/test_hip_parity.py), and holds where the pair is well conditioned:
``sum w mt^2 / sum w m^2 >= 1e-8`` in the statement, which :func:`reference` asserts for EVERY pair it returns.

Cubes: at nx >= 300 the grid and spectra of ``gen.muse_like`` with templates from the default prior; below that the
lines of that grid fall between channels (the ratio drops to 1e-19: the conditioning of ``1 + tiny``), so
``x = linspace(0, 1, nx)`` with templates ``1 + a exp(-0.5 ((x - mu) / sigma)^2)``, sigma at least two channel steps.
"""
import numpy as np

from massivedatans_amd import continuum, gen, musefuse

RTOL_L = 1e-11
MIN_RATIO = 1e-8


def broad_templates(x, B, rng):
    """``1 + a exp(-0.5 ((x - mu) / sigma)^2)`` on ``x`` in [0, 1], sigma of two to four channel steps."""
    step = 1.0 / max(len(x) - 1, 1)
    a = rng.uniform(0.5, 3.0, size=(B, 1))
    mu = rng.uniform(0.2, 0.8, size=(B, 1))
    sigma = rng.uniform(2.0, 4.0, size=(B, 1)) * step
    return 1.0 + a * np.exp(-0.5 * ((x[None, :] - mu) / sigma) ** 2)


def small_cube(nx, ndata, P, rng):
    """A cube on ``linspace(0, 1, nx)``: one broad line per spectrum times a scale, a polynomial of P terms, noise."""
    x = np.linspace(0.0, 1.0, nx)
    truth = broad_templates(x, ndata, rng)
    scale = 10 ** rng.uniform(-1, 1, size=(ndata, 1))
    coef = scale * rng.normal(size=(ndata, P))
    v = rng.uniform(0.5, 2.0, size=(ndata, nx)) * gen.NOISE_LEVEL ** 2
    y = scale * truth + coef @ continuum.legendre_basis(x, P) + rng.normal(size=(ndata, nx)) * np.sqrt(v)
    return dict(x=x, y=np.ascontiguousarray(y.T), v=np.ascontiguousarray(v.T))


def nonuniform_cube(nx, ndata, P, rng):
    """The recipe of gen.muse_like on ``sort(uniform)`` channels of its wavelength range."""
    x = np.sort(rng.uniform(4750, 9350, size=nx))
    z = rng.uniform(0.0, 0.02, size=ndata)
    scale = 10 ** rng.uniform(-1, 1, size=ndata)
    coef = scale[:, None] * np.array((1.0, 1.0, 0.5, 0.25)[:P]) * rng.normal(size=(ndata, P))
    v = rng.uniform(0.5, 2.0, size=(ndata, nx)) * gen.NOISE_LEVEL ** 2
    truth = np.array([s * gen.muse_template(x, (0.0, zz, 0.0, 1.0, 1.0)) for s, zz in zip(scale, z)])
    y = truth + coef @ continuum.legendre_basis(x, P) + rng.normal(size=(ndata, nx)) * np.sqrt(v)
    return dict(x=x, y=np.ascontiguousarray(y.T), v=np.ascontiguousarray(v.T))


def case(nx, ndata, P, B, seed=0, kind="muse"):
    """-> dict(x, y, v, ypred[B, nx], params[B, 5] or None).  ``kind``: "muse" (gen.muse_like with a continuum of
    P terms; "small" below nx = 300), "nonuniform", "masked" (a block of 40 channels at v = 1e30)."""
    rng = np.random.RandomState([nx, ndata, P, B, seed])
    if kind == "nonuniform":
        d = nonuniform_cube(nx, ndata, P, rng)
    elif nx < 300:
        d = small_cube(nx, ndata, P, rng)
    else:
        d = gen.muse_like(ndata, nx, continuum=P)
        d = dict(x=d["x"], y=d["y"], v=d["v"])
    if kind == "masked":
        d["v"] = d["v"].copy()
        d["v"][nx // 3:nx // 3 + 40, :] = 1e30
    if nx < 300:
        d["params"], d["ypred"] = None, broad_templates(d["x"], B, rng)
    else:
        d["params"] = musefuse.priortransform_batch(rng.uniform(size=(B, 5)))
        d["ypred"] = np.array([gen.muse_template(d["x"], p) for p in d["params"]])
    return d


def selection(ndata, sparse, rng):
    """None (all spectra), or a sparse one: an odd count, the last row among them."""
    if not sparse:
        return None
    count = max(1, (ndata // 2) | 1) if ndata > 1 else 1
    others = rng.choice(ndata - 1, size=count - 1, replace=False) if count > 1 else np.zeros(0, dtype=int)
    return np.sort(np.concatenate((others, [ndata - 1]))).astype(np.int32)


def reference(x, y, v, ypred, P, rows=None):
    """``(L, s, coef)`` of the longdouble statement; asserts the conditioning of every pair."""
    L, s, coef, ratio = continuum.Statement(x, y, v, P, rows, np.longdouble).score(ypred)
    assert np.all(ratio >= MIN_RATIO), ("ill-conditioned pair", float(ratio.min()))
    return L, s, coef


def rel_err(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want) / np.abs(want)))


class Hidden(object):
    """A MuseSpectra handle that is not recognised as one: ``MuseProblem`` and ``HostJointState`` then take the numpy
    route over it, scoring with the same device kernel."""

    def __init__(self, spectra):
        self.spectra = spectra
        self.continuum, self.lines, self.ref = spectra.continuum, spectra.lines, spectra.ref
        self.ncalls = 0

    def loglike_batch(self, ypred, data_mask=None):
        self.ncalls += 1
        return self.spectra.loglike_batch(ypred, data_mask)

    def loglike_batch_lines(self, params, data_mask=None):
        self.ncalls += 1
        return self.spectra.loglike_batch_lines(params, data_mask)
