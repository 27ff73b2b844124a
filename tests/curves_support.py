"""Test helper for the caller-defined models (tests/test_curves_host.py, tests/test_curves.py and the tests of the
other curve statistics): a Gaussian line written as a model of curves, the numpy statements of the two likelihoods,
and what the device tests of every statistic share -- a device entry point driven on padded rows, the selections,
a refusal, the joint state fed parameters in chunks, the problem on the numpy statement."""
import numpy as np

from massivedatans_amd import _host, _lib, gen, problem, sample


def line_model(x):
    """``model(xs[B, 3]) -> curves[B, nx]`` for rows (A, mu, log10 sig) after sample.priortransform_batch.  Every
    curve is computed by itself, so a candidate's curve does not depend on the batch it arrives in."""
    x = np.ascontiguousarray(x, dtype=float)

    def model(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        sig = _host.pow10(xs[:, 2])
        out = np.empty((len(xs), len(x)))
        for b in range(len(xs)):
            out[b] = xs[b, 0] * np.exp(-0.5 * ((xs[b, 1] - x) / sig[b]) ** 2)
        return out
    return model


class NumpyFixedNoise(object):
    """``loglike_batch(curves[B, nx], mask)``: the statement of sample.py:64-71 over ``y[nx, ndata]``."""

    def __init__(self, y, noise_level):
        self.y, self.noise = np.ascontiguousarray(y, dtype=float), float(noise_level)
        self.ndata = self.y.shape[1]

    def loglike_batch(self, curves, data_mask=None):
        c = np.atleast_2d(np.asarray(curves, dtype=float))
        y = self.y if data_mask is None else self.y[:, np.asarray(data_mask)]
        return -0.5 * (((c[:, :, None] - y[None]) / self.noise) ** 2).sum(axis=1)


class NumpyScaleMarginalised(object):
    """``loglike_batch(curves[B, nx], mask)``: the scale-marginalised chi^2 of cmuselike.c:45-64 over ``y``, ``v``
    of shape ``[nx, ndata]``: the best amplitude per spectrum, ``s = sum(y c / v) / (1e-10 + sum(c^2 / v))``,
    then ``-0.5 sum((y - s c)^2 / v)``."""

    def __init__(self, y, v):
        self.y, self.v = np.ascontiguousarray(y, dtype=float), np.ascontiguousarray(v, dtype=float)
        self.ndata = self.y.shape[1]

    def loglike_batch(self, curves, data_mask=None):
        c = np.atleast_2d(np.asarray(curves, dtype=float))[:, :, None]
        sel = slice(None) if data_mask is None else np.asarray(data_mask)
        y, v = self.y[None, :, sel], self.v[None, :, sel]
        s = (y * c / v).sum(axis=1) / (1e-10 + (c ** 2 / v).sum(axis=1))
        return -0.5 * (((y - s[:, None, :] * c) ** 2) / v).sum(axis=1)


def muse_cut(ndata, nx):
    """gen's MUSE-style data cut to ``ndata`` spectra x ``nx`` channels around the strongest line."""
    d = gen.muse_like(ndata, 4096)
    lo = int(np.searchsorted(d["x"], 5006.8 * 1.01)) - nx // 2
    return dict(x=np.ascontiguousarray(d["x"][lo:lo + nx]), y=np.ascontiguousarray(d["y"][lo:lo + nx]),
                v=np.ascontiguousarray(d["v"][lo:lo + nx]))


def muse_line_model(x):
    """``model(xs[B, 3]) -> curves[B, nx]``: one line on a flat continuum, rows (log_amp, z, log_width)."""
    x = np.ascontiguousarray(x, dtype=float)

    def model(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        out = np.empty((len(xs), len(x)))
        for b, (la, z, lw) in enumerate(xs):
            out[b] = 1.0 + 10 ** la * np.exp(-0.5 * ((x - 5006.8 * (1 + z)) / (4.0 * 10 ** lw)) ** 2)
        return out
    return model


def muse_prior(us):
    us = np.asarray(us, dtype=float)
    return np.column_stack((2.0 * us[:, 0] - 1.0, 0.02 * us[:, 1], us[:, 2] - 0.5))


gauss_prior = sample.priortransform_batch

# the tile kernels of 32-channel stages (fixed noise, fixed-scale chi^2) at their edges: nx across the stages, ndata
# across the 64 spectra of a wave and the 128 of a workgroup, B across a wave's 8 and a workgroup's 32 candidates
STAGE_EDGE_NX = (1, 2, 31, 32, 33, 63, 64, 65, 200, 513)
STAGE_EDGE_NDATA = (1, 63, 64, 65, 127, 128, 129, 300)
STAGE_EDGE_BS = (1, 7, 8, 9, 31, 32, 33, 70)
# 30 cases: every nx three times, every ndata and every B at least three times, paired (no product)
STAGE_EDGE_CASES = [(STAGE_EDGE_NX[i % 10], STAGE_EDGE_NDATA[(3 * i + i // 8) % 8], STAGE_EDGE_BS[(5 * i + 2 * (i // 8)) % 8])
                    for i in range(30)]


def dev_batch(lib, spectra, curves, pad, rows, fn, extra=(), per=1):
    """The device entry point ``fn`` on rows of nx + pad doubles (NaN behind the curves); ``extra``: its arguments
    between B and the row ids (the fixed-noise one takes the noise level there); ``per``: outputs per pair."""
    B, nx = curves.shape
    ldc = nx + pad
    wide = np.full((B, ldc), np.nan)
    wide[:, :nx] = curves
    M = spectra.ndata if rows is None else len(rows)
    out = np.empty((B, M, per)) if per > 1 else np.empty((B, M))
    d_c, d_o = lib.mdns_dev_alloc(wide.nbytes), lib.mdns_dev_alloc(out.nbytes)
    d_r = None
    try:
        assert d_c and d_o
        _lib.check(lib.mdns_h2d(d_c, _lib.ptr(wide), wide.nbytes), "h2d")
        if rows is not None:
            r32 = np.ascontiguousarray(rows, dtype=np.int32)
            d_r = lib.mdns_dev_alloc(r32.nbytes)
            _lib.check(lib.mdns_h2d(d_r, _lib.ptr(r32), r32.nbytes), "h2d")
        _lib.check(getattr(lib, fn)(spectra.handle, d_c, ldc, B, *(tuple(extra) + (d_r, M, d_o))), fn)
        _lib.check(lib.mdns_d2h(_lib.ptr(out), d_o, out.nbytes), "d2h")
    finally:
        for p in (d_c, d_o, d_r):
            if p:
                lib.mdns_dev_free(p)
    return out


def selections_by_size(ndata, rng):
    """All, the middle one, 63, 64 and 65 at random where there are more, every third."""
    sel = [("all", None), ("one", np.array([ndata // 2]))]
    for n in (63, 64, 65):
        if ndata > n:
            sel.append((str(n), np.sort(rng.choice(ndata, size=n, replace=False))))
    if ndata >= 3:
        sel.append(("third", np.arange(rng.randint(0, 3), ndata, 3)))
    return sel


def selections(ndata, rng, sparse=()):
    """All, one, every third, all but one (127 of 128, 128 of 129 ...), and ``m`` at random for every m of ``sparse``
    that leaves two out."""
    sel = [("all", None), ("one", np.array([ndata // 3]))]
    if ndata >= 3:
        sel.append(("third", np.arange(rng.randint(0, 3), ndata, 3)))
    if ndata > 1:
        sel.append(("ragged", np.sort(rng.choice(ndata, size=ndata - 1, replace=False))))
    for m in sparse:
        if ndata > m + 1:
            sel.append(("sparse %d" % m, np.sort(rng.choice(ndata, size=m, replace=False))))
    return sel


def refused(rc, *words):
    msg = _lib.last_error()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


class Chunks(object):
    """A joint state whose ``draw`` takes model parameters, goes through ``draw_params`` and -- ``noisy`` -- adds
    a noise block [B, M], the same one for the same call number."""

    def __init__(self, state, to_params, noisy, scorer=None):
        self.__dict__.update(_s=state, _p=to_params, _noisy=noisy, _scorer=scorer, _calls=0)

    def __getattr__(self, name):
        return getattr(self._s, name)

    def draw(self, xs, rows):
        self.__dict__["_calls"] += 1
        M = self._s.ndata if rows is None else len(rows)
        noise = np.random.RandomState(self._calls).normal(0, 1e-5, size=(len(xs), M)) if self._noisy else None
        params = self._p(xs)
        if self._scorer is not None:
            mask = np.zeros(self._s.ndata, dtype=bool)
            mask[np.arange(self._s.ndata) if rows is None else rows] = True
            self._scorer.begin(params, mask)
        return self._s.draw_params(params, rows, jitter=noise)


class StatementProblem(problem.CurveProblem):
    """The same problem with the numpy statement of the joint state over the device's curve kernel."""

    def _on_device(self):
        return False
