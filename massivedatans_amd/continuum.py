"""A polynomial continuum per spectrum, profiled out of the scale-marginalised likelihood: the numpy
statement of what ``csrc/mdns_continuum.hip`` computes (include/mdns.h Part 8), and a CPU backend over it.

With ``w = 1/v`` and the basis ``b_k(x_j) = Legendre P_k(t_j)``, ``k < P``,
``t_j = (2 x_j - x_0 - x_last) / (x_last - x_0)``:

* once per spectrum: ``G = sum_j w b b^T``, ``beta = G^-1 sum_j w b y``, ``yt = y - sum_k beta_k b_k``;
* per (template ``m``, spectrum): ``alpha = G^-1 sum_j w b m``, ``mt = m - sum_k alpha_k b_k``,
  ``s = sum w yt mt / (1e-10 + sum w mt^2)``, ``L = -0.5 sum w (yt - s mt)^2``.

That is the weighted least-squares minimum over ``(s, c_0..c_{P-1})`` of
``sum w (y - s m - sum_k c_k b_k)^2`` with the reference's ``1e-10`` (cmuselike.c:52,57) on the part of the
template the basis cannot express; the fitted continuum is ``c = beta - s alpha``.  The order is the
definition: residualise, sum, form the residual -- not ``q0 - a^2/c``, which cancels (at S/N 1000
``sum w y^2`` is 1e4 times chi^2).
"""
import numpy

MAX_TERMS = 4                                # include/mdns.h mdns_spectra_set_continuum


def check_terms(P):
    """``P`` as int; ValueError unless it is an integer in 0..MAX_TERMS."""
    if isinstance(P, bool) or not isinstance(P, (int, numpy.integer)) or not 0 <= int(P) <= MAX_TERMS:
        raise ValueError("continuum = %r must be an integer in 0..%d (terms of the polynomial; 0: none)" % (P, MAX_TERMS))
    return int(P)


def legendre_basis(x, P, dtype=float):
    """``b[P, nx]``: Legendre ``P_0..P_{P-1}`` at the channels ``x`` mapped linearly onto [-1, 1] (from ``x``,
    not from the channel index: grids need not be uniform), by the recurrence the device uses."""
    x = numpy.asarray(x, dtype=dtype)
    P = int(P)
    span = x[-1] - x[0]
    t = (2 * x - x[0] - x[-1]) / span if span != 0 else numpy.zeros_like(x)
    b = numpy.empty((P, len(x)), dtype=dtype)
    three = numpy.asarray(3, dtype=dtype)
    if P > 0:
        b[0] = 1
    if P > 1:
        b[1] = t
    if P > 2:
        b[2] = (3 * t * b[1] - 1) / 2
    if P > 3:
        b[3] = (5 * t * b[2] - 2 * b[1]) / three
    return b


def _cholesky(G):
    """Lower factors of ``G[M, P, P]`` in G's dtype; ValueError names the first spectrum with a pivot <= 0."""
    P = G.shape[-1]
    L = numpy.zeros_like(G)
    for k in range(P):
        for i in range(k + 1):
            v = G[:, k, i] - (L[:, k, :i] * L[:, i, :i]).sum(axis=-1)
            if i == k:
                if not numpy.all(v > 0):
                    raise ValueError("spectrum %d has fewer than %d channels with weight" % (int(numpy.argmin(v > 0)), P))
                L[:, k, k] = numpy.sqrt(v)
            else:
                L[:, k, i] = v / L[:, i, i]
    return L


def _chol_solve(L, rhs):
    """``G^-1 rhs`` for ``rhs[..., M, P]`` through the two triangular solves."""
    P = L.shape[-1]
    z = numpy.array(rhs, dtype=L.dtype)
    for k in range(P):
        for i in range(k):
            z[..., k] -= L[:, k, i] * z[..., i]
        z[..., k] /= L[:, k, k]
    for k in range(P - 1, -1, -1):
        for i in range(k + 1, P):
            z[..., k] -= L[:, i, k] * z[..., i]
        z[..., k] /= L[:, k, k]
    return z


class Statement(object):
    """The per-spectrum half of the definition for the spectra ``rows`` of ``y``, ``v`` ``[nx, ndata]`` (the
    reference's layout), in ``dtype``; :meth:`score` is the per-template half."""

    def __init__(self, x, y, v, P, rows=None, dtype=float):
        self.P = check_terms(P)
        if self.P < 1:
            raise ValueError("a continuum has 1 to %d terms" % MAX_TERMS)
        self.dtype = dtype
        self.b = legendre_basis(x, self.P, dtype)
        y = numpy.asarray(y).T
        v = numpy.asarray(v).T
        if rows is not None:
            y, v = y[rows], v[rows]
        self.y = numpy.asarray(y, dtype=dtype)
        self.w = 1 / numpy.asarray(v, dtype=dtype)
        if self.y.shape[1] < self.P:
            raise ValueError("spectrum 0 has %d channels, fewer than the %d terms" % (self.y.shape[1], self.P))
        G = numpy.einsum('mj,kj,lj->mkl', self.w, self.b, self.b)
        self.chol = _cholesky(G)
        self.beta = _chol_solve(self.chol, numpy.einsum('mj,kj->mk', self.w * self.y, self.b))
        self.yt = self.y - self.beta @ self.b

    def score(self, ypred, sel=None):
        """``ypred[B, nx]`` against the spectra ``sel`` (indices into this statement's rows; None: all) ->
        ``L[B, M]``, ``s[B, M]``, ``coef[B, M, P]`` and ``ratio[B, M] = sum w mt^2 / sum w m^2``, how much of the
        template the basis cannot express (the conditioning of the pair)."""
        ypred = numpy.atleast_2d(numpy.asarray(ypred, dtype=self.dtype))
        pick = (lambda a: a) if sel is None else (lambda a: a[sel])
        w, yt, beta, chol = pick(self.w), pick(self.yt), pick(self.beta), pick(self.chol)
        B, M = len(ypred), len(w)
        L = numpy.empty((B, M), dtype=self.dtype)
        s = numpy.empty((B, M), dtype=self.dtype)
        ratio = numpy.empty((B, M), dtype=self.dtype)
        coef = numpy.empty((B, M, self.P), dtype=self.dtype)
        for i, m in enumerate(ypred):
            wm = w * m
            alpha = _chol_solve(chol, wm @ self.b.T)
            mt = m - alpha @ self.b
            wmt = w * mt
            c = (wmt * mt).sum(axis=-1)
            s[i] = (wmt * yt).sum(axis=-1) / (1e-10 + c)
            r = yt - s[i][:, None] * mt
            L[i] = -0.5 * (w * r * r).sum(axis=-1)
            coef[i] = beta - s[i][:, None] * alpha
            with numpy.errstate(divide='ignore', invalid='ignore'):
                ratio[i] = c / (wm * m).sum(axis=-1)
        return L, s, coef, ratio


def loglike_statement(x, y, v, ypred, P, rows=None, dtype=float):
    """The definition, vectorised: ``x[nx]``, ``y`` / ``v`` ``[nx, ndata]``, templates ``ypred[B, nx]``, ``rows``
    the selected spectra (None: all) -> ``L[B, M]``, ``s[B, M]``, ``coef[B, M, P]`` in ``dtype``."""
    return Statement(x, y, v, P, rows, dtype).score(ypred)[:3]


def _rows(data_mask, ndata):
    if data_mask is None:
        return None
    m = numpy.asarray(data_mask)
    if m.dtype == numpy.bool_:
        if m.shape != (ndata,):
            raise ValueError("data_mask has shape %s, expected (%d,)" % (m.shape, ndata))
        return None if m.all() else numpy.flatnonzero(m)
    return m.astype(int)


class ContinuumScorer(object):
    """The CPU backend of a MUSE-style problem with a continuum (``MuseProblem(backend=...)``, and through it
    :class:`massivedatans_amd.jointstate.HostJointState`): ``loglike_batch(ypred[B, nx], data_mask) -> L[B, M]``
    by the float64 statement, ``loglike_batch_lines(params, data_mask)`` over the templates of ``lines``
    (:func:`massivedatans_amd.gen.muse_template`; None: the built-in three)."""

    def __init__(self, x, y, v, P, lines=None, ref=1):
        from . import gen
        self.x = numpy.ascontiguousarray(x, dtype=float)
        self.statement = Statement(self.x, y, v, P)
        self.continuum = self.statement.P
        self.ndata, self.nx = self.statement.y.shape
        self.lines, self.ref = (None, 1) if lines is None else gen.check_lines(lines, ref)

    def fit_batch(self, ypred, data_mask=None):
        """-> ``(L, s, coef)``"""
        ypred = numpy.atleast_2d(numpy.asarray(ypred, dtype=float))
        if ypred.shape[1] != self.nx:
            raise ValueError("templates must be [B, %d]" % self.nx)
        return self.statement.score(ypred, _rows(data_mask, self.ndata))[:3]

    def loglike_batch(self, ypred, data_mask=None):
        return self.fit_batch(ypred, data_mask)[0]

    def loglike_batch_lines(self, params, data_mask=None):
        from . import gen
        lines = gen.MUSE_LINES if self.lines is None else self.lines
        params = numpy.atleast_2d(numpy.asarray(params, dtype=float))
        ypred = numpy.array([gen.muse_template(self.x, p, lines, self.ref) for p in params]).reshape(len(params), self.nx)
        return self.loglike_batch(ypred, data_mask)


__all__ = ['legendre_basis', 'loglike_statement', 'Statement', 'ContinuumScorer', 'check_terms', 'MAX_TERMS']
