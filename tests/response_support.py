"""Test helper for the instrument response (tests/test_response_host.py, tests/test_response.py): the sequential
statement, responses that stress the device layout, the bound against a dense product, the device fold driven on padded
rows, and the spectra, model and parameters the draw tests share.

THE BOUND against ``dense = curves @ R.T`` (numpy's product: any order, any contraction).  With ``u = 2**-53`` and
``gamma(n) = n u / (1 - n u)`` (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1): a sum of ``n``
products formed in ANY order, each product rounded or fused, differs from the exact sum by at most
``gamma(n) * sum |a_i| |b_i|`` (Lemma 3.1 / eq. 3.5: every term carries at most one rounding of its product and n - 1 of
the additions it takes part in).  ``Response.statement`` sums the ``len_j`` entries of row ``j``; the dense product sums
``n_in`` terms of which ``n_in - len_j`` are exact zeros that change no partial sum, but ``gamma(n_in)`` holds whatever
BLAS does with them.  Both errors are against the same exact sum, and ``sum |vals| |curve|`` over the row is
``(|curves| @ |R|.T)[b][j]``, so

    |statement - dense| <= (gamma(len_j) + gamma(n_in)) * (|curves| @ |R|.T)

with nothing fitted to what the code under test gives."""
import numpy as np

from massivedatans_amd import _lib
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, MuseSpectra, WeightedSpectra
from massivedatans_amd.response import Response
from massivedatans_amd.tablemodel import TableModel
from curves_support import gauss_prior

U = 2.0 ** -53


def gamma(n):
    n = np.asarray(n, dtype=float)
    return n * U / (1.0 - n * U)


def dense_bound(resp, curves):
    """[B, nx]: the bound of the module docstring."""
    lens = np.diff(resp.rowptr)
    return (gamma(lens) + gamma(resp.n_in))[None, :] * (np.abs(curves) @ np.abs(resp.dense()).T)


def sequential(resp, curves):
    """include/mdns.h Part 13 as written: a Python loop per candidate, per channel, per entry."""
    curves = np.atleast_2d(np.asarray(curves, dtype=float))
    out = np.empty((len(curves), resp.nx))
    with np.errstate(all="ignore"):
        for b in range(len(curves)):
            for j in range(resp.nx):
                acc = np.float64(0.0)
                for p in range(resp.rowptr[j], resp.rowptr[j + 1]):
                    acc = acc + resp.vals[p] * curves[b, resp.cols[p]]
                out[b, j] = acc
    return out


def from_rows(rows, n_in, x_in=None):
    """``rows``: per channel ``(cols ascending, vals)``."""
    rowptr = np.concatenate(([0], np.cumsum([len(c) for c, _ in rows]))).astype(np.int64)
    cols = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if rows else np.zeros(0, dtype=np.int32)
    vals = np.concatenate([np.asarray(v, dtype=float) for _, v in rows]) if rows else np.zeros(0)
    return Response(rowptr, cols.astype(np.int32), vals, n_in, x_in=x_in)


def random_response(rng, nx, n_in, most=40):
    """Signed values, scattered (non-banded) columns, rows of 0 to ``most`` entries."""
    rows = []
    for _ in range(nx):
        n = int(rng.randint(0, min(most, n_in) + 1))
        rows.append((np.sort(rng.choice(n_in, size=n, replace=False)), rng.normal(size=n)))
    return from_rows(rows, n_in)


def stress_response(rng, nx, n_in):
    """:func:`random_response` with the rows that stress the layout of csrc/mdns_response.hip planted where ``nx`` has
    room for them: lengths 0, 1, 17 and ``n_in`` inside one wave (channels 3 .. 6), a row of one entry (1), a full row
    (2), a group of 64 channels with only empty rows (64 .. 127), an empty first and last channel.  Returns the response
    and the names of what was planted."""
    r = random_response(rng, nx, n_in)
    rows = [(r.cols[r.rowptr[j]:r.rowptr[j + 1]], r.vals[r.rowptr[j]:r.rowptr[j + 1]]) for j in range(nx)]
    planted = []

    def plant(j, n, name):
        if j < nx:
            n = min(n, n_in)
            rows[j] = (np.sort(rng.choice(n_in, size=n, replace=False)), -np.abs(rng.normal(size=n)) if name == "negative" else rng.normal(size=n))
            planted.append(name)
    plant(1, 1, "one entry")
    plant(2, n_in, "full row")
    for j, n in ((3, 0), (4, 1), (5, 17), (6, n_in)):
        plant(j, n, "wave length %d" % min(n, n_in))
    plant(7, 5, "negative")
    if nx >= 129:
        for j in range(64, 128):
            rows[j] = (np.zeros(0, dtype=np.int32), np.zeros(0))
        planted.append("empty group")
    plant(0, 0, "empty first")
    plant(nx - 1, 0, "empty last")
    return from_rows(rows, n_in), planted


def lsf_response(nx, n_in, sigma_bins, x_in=None, cut=3.0):
    """A Gaussian line-spread function cut at ``cut`` sigma, normalised per bin before the cut: channel ``j`` sits at
    bin ``j (n_in - 1) / (nx - 1)``; about ``2 cut sigma_bins`` entries per row, all positive."""
    centre = np.arange(nx) * ((n_in - 1) / max(nx - 1, 1))
    rows = []
    for j in range(nx):
        lo, hi = max(0, int(np.ceil(centre[j] - cut * sigma_bins))), min(n_in - 1, int(np.floor(centre[j] + cut * sigma_bins)))
        c = np.arange(lo, hi + 1)
        rows.append((c, np.exp(-0.5 * ((c - centre[j]) / sigma_bins) ** 2) / (sigma_bins * np.sqrt(2 * np.pi)) * (n_in / nx)))
    return from_rows(rows, n_in, x_in=x_in)


def dev_fold(lib, dr, curves, pad_in=0, pad_out=0, sentinel=-7.25):
    """``mdns_response_fold_batch_dev`` on input rows of n_in + pad_in doubles (NaN behind the curves) into output rows
    of nx + pad_out doubles pre-filled with ``sentinel``: the folded curves [B, nx] and whether the output padding still
    holds the sentinel."""
    curves = np.atleast_2d(np.ascontiguousarray(curves, dtype=float))
    B = len(curves)
    ldc, ldo = dr.n_in + pad_in, dr.nx + pad_out
    wide_in = np.full((B, ldc), np.nan)
    wide_in[:, :dr.n_in] = curves
    wide_out = np.full((B, ldo), sentinel)
    d_c, d_o = lib.mdns_dev_alloc(wide_in.nbytes), lib.mdns_dev_alloc(wide_out.nbytes)
    try:
        assert d_c and d_o
        _lib.check(lib.mdns_h2d(d_c, _lib.ptr(wide_in), wide_in.nbytes), "h2d")
        _lib.check(lib.mdns_h2d(d_o, _lib.ptr(wide_out), wide_out.nbytes), "h2d")
        _lib.check(lib.mdns_response_fold_batch_dev(dr.handle, d_c, ldc, B, d_o, ldo), "mdns_response_fold_batch_dev")
        _lib.check(lib.mdns_d2h(_lib.ptr(wide_out), d_o, wide_out.nbytes), "d2h")
    finally:
        for p in (d_c, d_o):
            if p:
                lib.mdns_dev_free(p)
    return np.ascontiguousarray(wide_out[:, :dr.nx]), bool((wide_out[:, dr.nx:] == sentinel).all())


# ---- what the draw tests share: model bins, channels, a positive table model on the bins, spectra of every statistic ----
NX, N_IN, NDATA = 33, 70, 70
STATS = ("noise", "marginal", "continuum", "chi2", "poisson", "wstat")


def bins_and_channels():
    x_in = np.linspace(420.0, 880.0, N_IN)
    x = np.linspace(420.0, 880.0, NX)
    return x, x_in


def draw_response():
    """33 channels x 70 bins, about 13 positive entries per row (count rates must stay >= 0)."""
    x, x_in = bins_and_channels()
    return lsf_response(NX, N_IN, 2.0, x_in=x_in)


def positive_model(seed=2):
    """A table of positive templates over two axes, with z and A (tests/test_table_model.py's)."""
    rng = np.random.RandomState(seed)
    a0, a1 = np.array([0.0, 0.3, 1.0, 1.6]), np.array([-1.0, 0.5, 1.0])
    grid = np.sort(np.concatenate(([350.0, 900.0], rng.uniform(350, 900, size=38))))
    width = (15.0 + 40.0 * a0)[:, None, None]
    table = 0.2 + (1.0 + 0.5 * a1[None, :, None]) * np.exp(-0.5 * ((grid[None, None, :] - 600.0) / width) ** 2)
    return TableModel([a0, a1], grid, table, redshift=True, amplitude=True)


def to_params(tm):
    """Rows of curves_support.gauss_prior as rows of the table model, from mu and log sigma alone (the faint lines that
    filter_support._drive turns to stay draws from the whole prior)."""
    a0, a1 = tm.axes

    def convert(xs):
        xs = np.atleast_2d(np.asarray(xs, dtype=float))
        u1, u2 = (xs[:, 1] - 400.0) / 400.0, xs[:, 2] / 2.0
        u3, u4 = (7.0 * u1 + 3.0 * u2) % 1.0, (13.0 * u1 + 5.0 * u2) % 1.0
        return np.ascontiguousarray(np.column_stack((a0[0] - 0.1 + (a0[-1] - a0[0] + 0.2) * u1, a1[0] - 0.1 + (a1[-1] - a1[0] + 0.2) * u2,
                                                     0.2 * u3, 0.5 * 100.0 ** u4)))
    return convert


def make_spectra(stat, tm, resp):
    """Spectra of ``NDATA`` folded truths under the statistic ``stat``, without a response attached; the same bytes for
    the same arguments."""
    x, x_in = bins_and_channels()
    rng = np.random.RandomState(5)
    truth = to_params(tm)(gauss_prior(rng.uniform(size=(NDATA, 3))))
    clean = resp.statement(tm.statement(x_in, truth)).T                    # [nx, ndata]
    if stat == "noise":
        return GaussLineSpectra(x, clean + 0.5 * rng.normal(size=clean.shape), noise_level=0.5)
    v = rng.uniform(0.1, 0.5, size=clean.shape)
    y = clean + np.sqrt(v) * rng.normal(size=clean.shape)
    if stat == "marginal":
        return MuseSpectra(x, y, v)
    if stat == "continuum":
        return MuseSpectra(x, y, v, continuum=2)
    if stat == "chi2":
        return WeightedSpectra(x, y, v)
    e = rng.uniform(0.5, 2.0, size=clean.shape)
    n = rng.poisson(clean * e).astype(float)
    if stat == "poisson":
        return CountSpectra(x, n, e)
    g = rng.uniform(1.0, 3.0, size=clean.shape)
    return CountSpectra(x, n + rng.poisson(0.3 * e), e, rng.poisson(0.3 * g).astype(float), g)
