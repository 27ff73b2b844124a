"""Synthetic inputs named by the benchmark configs.

These restate the RNG call ORDER of the reference generators so that the arrays are
bit-identical to what the reference scripts write (numpy legacy ``RandomState`` streams are
frozen by numpy's compatibility policy):

* :func:`horns`   <- gensimple_horns.py:15-39  (``data_widths_N.hdf5``: datasets ``x``, ``y``)
* :func:`nothing` <- gennothing.py:7-12        (``data_nothing_N.hdf5``)
* :func:`muse_like` has no generator in the reference (musefuse.py:31-154 reads a real MUSE
  cube); it is the synthetic stand-in SURVEY.md section 8(d) defines for config C5.

The reference stores ``y`` as ``[n_channels, n_datasets]`` (C order); that is what these
functions return, so they can be fed to the drop-in ``like()`` entry points unchanged.  The
device-resident layout ``[n_datasets, n_channels]`` is produced at upload time
(:class:`massivedatans_amd.like.GaussLineSpectra`).

File containers: a path ending in ``.hdf5`` / ``.h5`` is read and written through h5py exactly as
the reference does (same dataset names, gzip + shuffle), so files of the reference's generators
can be fed in directly -- where h5py is installed.  It is not in this image (nor on the GPU
box), so everything here and in the tests uses ``.npz`` with the reference's dataset names.
"""
import numpy as np

#: wavelength grid of the toy problem (gensimple_horns.py:15, gennothing.py:7)
N_CHANNELS = 200
NOISE_LEVEL = 0.01   # gensimple_horns.py:26, sample.py:45
REST_WAVE = 656      # gensimple_horns.py:21
LINE_WIDTH = 5.0     # gensimple_horns.py:23


def wavelength_grid():
    return np.linspace(400, 800, N_CHANNELS)


def horns(n):
    """``gensimple_horns.py N``: one narrow emission line per spectrum, redshifts piling up in
    two "horns".  Returns ``dict(x, y, z, mean_narrow, width_narrow, height_narrow)`` with
    ``y`` of shape ``[200, n]``.

    RNG order (gensimple_horns.py:19-39): ``seed(n)``; ``uniform(-pi, pi, n)``;
    ``power(3, n)``; then, spectrum by spectrum, ``normal(0, 0.01, 200)``.
    """
    n = int(n)
    x = wavelength_grid()
    rng = np.random.RandomState(n)          # numpy.random.seed(N) on the global stream
    z = np.arctan(rng.uniform(-np.pi, np.pi, size=n)) * 0.1
    centre = REST_WAVE * (1 + z)
    width = LINE_WIDTH * np.ones(n)
    height = 0.02 / rng.power(3, size=n)
    # noiseless lines, built [n, 200] then transposed exactly as gensimple_horns.py:8-13,31-32
    clean = height.reshape((-1, 1)) * np.exp(
        -0.5 * ((centre.reshape((-1, 1)) - x.reshape((1, -1))) / width.reshape((-1, 1))) ** 2)
    y = np.transpose(clean).copy()
    for i in range(n):                      # column-by-column draw order matters
        y[:, i] += rng.normal(0, NOISE_LEVEL, size=len(x))
    return dict(x=x, y=np.ascontiguousarray(y), z=z, mean_narrow=centre, width_narrow=width,
                height_narrow=height)


def nothing(n):
    """``gennothing.py N``: pure noise spectra (low-acceptance RadFriends stress)."""
    n = int(n)
    x = wavelength_grid()
    rng = np.random.RandomState(n)
    y = rng.normal(0, NOISE_LEVEL, size=(len(x), n))
    return dict(x=x, y=np.ascontiguousarray(y))


# --- MUSE-style synthetic cube (config C5) -------------------------------

#: rest wavelengths [Angstrom], relative amplitudes and widths of the three template lines
MUSE_LINES = ((4861.3, 0.35, 4.0), (5006.8, 1.0, 4.0), (6562.8, 0.8, 5.0))


#: lines a list may hold at most (include/mdns.h mdns_spectra_set_lines)
MAX_LINES = 6


def check_lines(lines, ref):
    """``lines`` as a tuple of G ``(mu, a, sigma)`` float rows and ``ref`` as int; ValueError unless
    1 <= G <= MAX_LINES, 0 <= ref < G, every value finite and every sigma > 0."""
    try:
        rows = tuple(tuple(float(v) for v in row) for row in lines)
    except (TypeError, ValueError):
        raise ValueError("lines must be rows of three numbers (mu, a, sigma)")
    if not 1 <= len(rows) <= MAX_LINES:
        raise ValueError("a line list has 1 to %d lines, not %d" % (MAX_LINES, len(rows)))
    for g, row in enumerate(rows):
        if len(row) != 3 or not all(np.isfinite(row)):
            raise ValueError("line %d: three finite numbers (mu, a, sigma) are needed, got %r" % (g, row))
        if not row[2] > 0:
            raise ValueError("line %d: sigma = %g must be positive" % (g, row[2]))
    if isinstance(ref, bool) or int(ref) != ref or not 0 <= int(ref) < len(rows):
        raise ValueError("ref = %r must be the index of one of the %d lines" % (ref, len(rows)))
    return rows, int(ref)


def muse_template(x, params, lines=MUSE_LINES, ref=1):
    """Gaussian emission lines on a flat continuum.  ``lines``: G rows ``(mu_g, A_g, sigma_g)``;
    ``params`` = (log_amp, z, log_width_scale, r_g for g != ref in ascending g): ``ypred = 1 +
    10**log_amp * sum_g r_g A_g exp(-0.5 ((x - mu_g (1+z)) / (sigma_g 10**log_width_scale))**2)``
    with ``r_ref = 1``.  The defaults are the three lines of config C5: (log_amp, z,
    log_width_scale, ratio1, ratio3).  Host statement of what the device template kernels
    evaluate (``mdns_lines_template_batch``)."""
    params = tuple(params)
    if len(params) != len(lines) + 2:
        raise ValueError("%d lines take %d parameters, not %d" % (len(lines), len(lines) + 2, len(params)))
    log_amp, z, log_ws = params[:3]
    ratios = params[3:3 + ref] + (1.0,) + params[3 + ref:]
    y = np.ones_like(x)
    for (mu, a, sg), r in zip(lines, ratios):
        y = y + (10 ** log_amp) * r * a * np.exp(-0.5 * ((x - mu * (1 + z)) / (sg * 10 ** log_ws)) ** 2)
    return y


def muse_like(n, nx=4096, lines=MUSE_LINES, ref=1, continuum=0):
    """Synthetic IFU cube: ``n`` spaxels x ``nx`` channels.  Returns ``dict(x, y, v, z, scale)``
    with ``y`` and ``v`` (per-pixel variance) of shape ``[nx, n]``, the layout cmuselike.c:54
    indexes (``i + j*ndata``).  The truth holds ``lines`` (all ratios 1).

    ``continuum=P`` (1..4) adds to spaxel ``i`` the polynomial ``sum_k scale_i a_k g[i, k] P_k(t)`` in the
    Legendre basis of :func:`massivedatans_amd.continuum.legendre_basis`, ``a = (1, 1, 0.5, 0.25)[:P]``,
    ``g = RandomState([n, P]).normal(size=(n, P))`` -- a stream of its own, so that ``continuum=0`` returns the
    same bytes as ever; the result gains ``continuum_coef`` ``[n, P]``."""
    n = int(n)
    x = np.linspace(4750, 9350, nx)
    rng = np.random.RandomState(n)
    z = rng.uniform(0.0, 0.02, size=n)
    scale = 10 ** rng.uniform(-1, 1, size=n)
    y = np.empty((nx, n))
    v = np.empty((nx, n))
    for i in range(n):
        truth = scale[i] * muse_template(x, (0.0, z[i], 0.0) + (1.0,) * (len(lines) - 1), lines, ref)
        v[:, i] = rng.uniform(0.5, 2.0, size=nx) * NOISE_LEVEL ** 2
        y[:, i] = truth + rng.normal(0, 1, size=nx) * np.sqrt(v[:, i])
    out = dict(x=x, y=y, v=v, z=z, scale=scale)
    if continuum:
        from . import continuum as _continuum
        P = _continuum.check_terms(continuum)
        g = np.random.RandomState([n, P]).normal(size=(n, P))
        coef = scale[:, None] * np.array((1.0, 1.0, 0.5, 0.25)[:P]) * g
        y += (coef @ _continuum.legendre_basis(x, P)).T
        out["continuum_coef"] = coef
    return out


def _is_hdf5(path):
    return str(path).endswith(('.hdf5', '.h5'))


def _h5py():
    try:
        import h5py
    except ImportError:
        raise RuntimeError("reading/writing .hdf5 needs h5py, which is not installed; "
                           "use a .npz file (gen.save / gen.load) instead")
    return h5py


def write_datasets(path, data):
    """``data``: name -> array.  ``.hdf5``: one gzip + shuffle dataset per name (scalars plain),
    as gensimple_horns.py:61-67 and sample.py:202-211 write them; otherwise a compressed .npz."""
    if _is_hdf5(path):
        with _h5py().File(path, 'w') as f:
            for k, v in data.items():
                v = np.asarray(v)
                if v.ndim == 0:
                    f.create_dataset(k, data=v)
                else:
                    f.create_dataset(k, data=v, compression='gzip', shuffle=True)
    else:
        np.savez_compressed(path, **data)


def read_datasets(path):
    if _is_hdf5(path):
        with _h5py().File(path, 'r') as f:
            return {k: np.asarray(f[k][()]) for k in f.keys()}
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def save(path, data):
    write_datasets(path, data)


def load(path, ndata=None):
    """Counterpart of sample.py:28-31: ``x`` and the first ``ndata`` columns of ``y``."""
    out = read_datasets(path)
    if ndata is not None:
        # (e: exposures of count spectra; b, eb: their background spectra and those exposures, sample.load_model)
        for k in ("y", "v", "e", "b", "eb"):
            if k in out and (k in ("y", "v") or np.ndim(out[k]) == 2):
                out[k] = np.ascontiguousarray(out[k][:, :int(ndata)])
    return out
