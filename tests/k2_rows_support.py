"""Case builders, the extended-precision statement and the launch rule for the tests of the exact K2 row kernels
(tests/test_k2_rows.py): ``k_muse_rows<NP, CB>``, ``k_muse_rows2<NP>`` and ``k_muse_rows_generic`` of csrc/mdns_like.hip.

The reference of every comparison is :func:`statement` in ``np.longdouble``: the definition of cmuselike.c:45-64 as the
kernels state it.  The same code at ``dtype=np.float64`` is the comparison point for tolerances: on the cubes of
:func:`case` it stays within 1e-15 of the longdouble one for every nx >= 255, 2e-14 at nx = 7 and 2e-13 at nx = 3, so the project's K2
figure, 1e-11 relative (continuum_support.RTOL_L), leaves the kernels four orders of magnitude and a wrong channel none.

Nothing here touches the device.
"""
import numpy as np

from massivedatans_amd import gen, musefuse
from continuum_support import RTOL_L, broad_templates, rel_err, selection, small_cube  # noqa: F401  (re-exported)

RTOL_SLOT = 1e-13       # one pair through two instantiations, or in the two places of a candidate pair: other reduction trees


def statement(y, v, ypred, rows=None, dtype=np.longdouble):
    """``L[B, M]`` for ``y``, ``v`` channel-major ``[nx, ndata]`` and templates ``ypred[B, nx]``:
    ``s = sum(y w m) / (1e-10 + sum(m m w))`` with ``w = 1 / v``, ``L = -0.5 sum((y - s m)^2 w)``; ``rows`` selects
    spectra (any order, repeats allowed)."""
    y, w = np.asarray(y, dtype=dtype).T, 1 / np.asarray(v, dtype=dtype).T
    if rows is not None:
        y, w = y[np.asarray(rows)], w[np.asarray(rows)]
    ypred = np.atleast_2d(np.asarray(ypred, dtype=dtype))
    L = np.empty((len(ypred), len(y)), dtype=dtype)
    yw = y * w
    for b, m in enumerate(ypred):
        s = (yw * m).sum(axis=1) / (dtype(1e-10) + (w * (m * m)).sum(axis=1))
        r = y - s[:, None] * m
        L[b] = dtype(-0.5) * (r * r * w).sum(axis=1)
    return L


def case(nx, ndata, B, seed=0):
    """-> dict(x, y, v, ypred[B, nx], params[B, 5] or None).  nx >= 300: the cube of ``gen.muse_like`` with templates
    from the default prior; below that the lines of that grid fall between channels (continuum_support.py), so
    ``small_cube`` with ``broad_templates``."""
    rng = np.random.RandomState([nx, ndata, B, seed])
    if nx < 300:
        d = small_cube(nx, ndata, 0, rng)
        d["params"], d["ypred"] = None, broad_templates(d["x"], B, rng)
        return d
    d = gen.muse_like(ndata, nx)
    d = dict(x=d["x"], y=d["y"], v=d["v"])
    d["params"] = musefuse.priortransform_batch(rng.uniform(size=(B, 5)))
    d["ypred"] = np.array([gen.muse_template(d["x"], p) for p in d["params"]])
    return d


def channel_blocks(nx):
    """NP of the row kernels: channel pairs per thread, 512 channels each -- ``ceil(nx / 512)`` exactly, so that the
    512 NP doubles a kernel reads of a template row are the ``model_ld(nx)`` doubles the row owns."""
    return max(1, -(-nx // 512))


def variant(B, M, num_cus):
    """``muse_rows_variant``: 2 two spectra per workgroup, 1 pairs of candidates, 0 one candidate."""
    if B >= 4 and M >= 2 * num_cus:
        return 2
    return 1 if B >= 2 else 0


def expected_kernel(nx, B, M, num_cus):
    """What ``mdns_profile_kernel(1)`` reports after ``launch_muse_rows`` scored B templates against M spectra."""
    if nx > 4096:
        return "k_muse_rows_generic"
    v = variant(B, M, num_cus)
    if v == 2:
        return "k_muse_rows2<%d>" % channel_blocks(nx)
    return "k_muse_rows<%d, %d>" % (channel_blocks(nx), 2 if v == 1 else 1)


def scrambled(ndata, rng):
    """``ndata`` row ids (as many as a call may name) in no order, with repeats, the last row among them."""
    ids = rng.randint(0, ndata, size=ndata)
    if ndata > 2:
        ids[1] = ndata - 1
        ids[0] = ids[ndata - 1]
    else:
        ids[rng.randint(ndata)] = ndata - 1
    return ids.astype(np.int32)
