"""The instrument response: model curves on fine bins, folded onto the data's channels before they are scored.

Count spectra of real instruments are not measured on the model's bins.  The model lives on ``n_in`` fine energy (or
wavelength) bins, the data on ``nx`` detector channels, and between the two sits a sparse, mostly banded matrix: RMF x
ARF in X-ray fitting, a wavelength-dependent line-spread function for a spectrograph.  :class:`Response` holds that
matrix; given to :class:`massivedatans_amd.problem.CurveProblem` as ``response=``, the model returns ``[B, n_in]`` and
every curve is folded on the device (``include/mdns.h`` Part 13, ``csrc/mdns_response.hip``) between the kernel that
makes it and the kernel that scores it -- the curves of a :class:`massivedatans_amd.tablemodel.TableModel` never leave
the GPU.

    import numpy
    from massivedatans_amd import problem, sample
    from massivedatans_amd.response import Response

    # the arrays of an RMF's MATRIX extension (the caller reads the FITS file) and the ARF's effective area
    rsp = Response.from_ogip(n_grp, f_chan, n_chan, matrix, n_channels=1024, first_channel=1, arf=specresp, x_in=e_mid)
    p = problem.CurveProblem(channels, counts, model, priortransform_batch, ndim=3, poisson=True, exposure=t, response=rsp)

One response is shared by all spectra of a run; a per-spectrum effective area goes into ``exposure``.

:meth:`Response.statement` is the same chain of single rounded float64 operations in numpy: the CPU path, and what the
device agrees with bit for bit.
"""
import numpy

from . import _lib

MAX_NX = 1 << 20                              # include/mdns.h MDNS_TABLE_MAX_NX
MAX_NNZ = 2 ** 31 - 1


class Response(object):
    """``nx = len(rowptr) - 1`` output channels and ``n_in`` model bins, in CSR by channel: ``rowptr`` i64[nx + 1] with
    ``rowptr[0] = 0``, non-decreasing, ``rowptr[nx] = nnz``; ``cols`` i32[nnz], strictly increasing inside a row, in
    ``[0, n_in)``; ``vals`` f64[nnz], finite, any sign.  Anything else raises ValueError, naming the array and the index
    (the rules and messages of ``mdns_response_create``).  ``x_in`` f64[n_in]: the abscissa of the model bins, what a
    :class:`massivedatans_amd.tablemodel.TableModel` is evaluated on."""

    def __init__(self, rowptr, cols, vals, n_in, x_in=None):
        rowptr = numpy.ascontiguousarray(rowptr, dtype=numpy.int64)
        if rowptr.ndim != 1 or len(rowptr) < 2:
            raise ValueError("rowptr must be a one-dimensional array of nx + 1 >= 2 entries, got shape %s" % (rowptr.shape,))
        nx, n_in = len(rowptr) - 1, int(n_in)
        if nx > MAX_NX:
            raise ValueError("nx=%d: 1 to %d channels" % (nx, MAX_NX))
        if not 1 <= n_in <= MAX_NX:
            raise ValueError("n_in=%d: 1 to %d bins" % (n_in, MAX_NX))
        if rowptr[0] != 0:
            raise ValueError("rowptr[0] = %d: must be 0" % rowptr[0])
        down = numpy.flatnonzero(numpy.diff(rowptr) < 0)
        if len(down):
            j = int(down[0])
            raise ValueError("rowptr[%d] = %d < rowptr[%d] = %d: rowptr must be non-decreasing" % (j + 1, rowptr[j + 1], j, rowptr[j]))
        nnz = int(rowptr[-1])
        if nnz > MAX_NNZ:
            raise ValueError("rowptr[%d] = %d: %d entries at most" % (nx, nnz, MAX_NNZ))
        cols_in = numpy.asarray(cols)
        if cols_in.ndim != 1 or len(cols_in) != nnz:
            raise ValueError("cols has shape %s, rowptr[%d] = %d entries are asked for" % (cols_in.shape, nx, nnz))
        if nnz and not numpy.issubdtype(cols_in.dtype, numpy.integer):
            raise ValueError("cols must hold integers, got %s" % cols_in.dtype)
        vals = numpy.ascontiguousarray(vals, dtype=float)
        if vals.ndim != 1 or len(vals) != nnz:
            raise ValueError("vals has shape %s, rowptr[%d] = %d entries are asked for" % (vals.shape, nx, nnz))
        lens = numpy.diff(rowptr)
        row_of = numpy.repeat(numpy.arange(nx), lens)                    # the channel of entry p
        outside = numpy.flatnonzero((cols_in < 0) | (cols_in >= n_in))
        if len(outside):
            p = int(outside[0])
            raise ValueError("cols[%d] = %d outside [0, %d) (channel %d)" % (p, cols_in[p], n_in, row_of[p]))
        cols = numpy.ascontiguousarray(cols_in, dtype=numpy.int32)
        if nnz > 1:
            same_row = row_of[1:] == row_of[:-1]
            back = numpy.flatnonzero(same_row & (cols[1:] <= cols[:-1]))
            if len(back):
                p = int(back[0]) + 1
                raise ValueError("cols[%d] = %d after %d: cols must be strictly increasing inside a row (channel %d)"
                                 % (p, cols[p], cols[p - 1], row_of[p]))
        bad = numpy.flatnonzero(~numpy.isfinite(vals))
        if len(bad):
            p = int(bad[0])
            raise ValueError("vals[%d] = %r is not finite (channel %d)" % (p, float(vals[p]), row_of[p]))
        if x_in is not None:
            x_in = numpy.ascontiguousarray(x_in, dtype=float)
            if x_in.shape != (n_in,):
                raise ValueError("x_in has shape %s, expected (%d,)" % (x_in.shape, n_in))
        self.rowptr, self.cols, self.vals, self.x_in = rowptr, cols, vals, x_in
        self.nx, self.n_in, self.nnz = nx, n_in, nnz
        self._lens = lens

    def statement(self, curves):
        """``curves[B, n_in] -> folded[B, nx]``: include/mdns.h Part 13 in numpy, vectorised over candidates and channels.
        Per channel ``acc = +0.0``, then over the positions ``l`` of its row ascending ``acc = acc + vals[p] *
        curves[:, cols[p]]``, each one rounded float64 operation.  The loop runs to the longest row; a row that has ended
        adds ``where(l < len_j, ..., 0.0)``: ``acc`` starts at ``+0.0`` and can never become ``-0.0``, so adding ``+0.0``
        changes nothing."""
        curves = numpy.asarray(curves, dtype=float)
        one = curves.ndim == 1
        curves = numpy.atleast_2d(curves)
        if curves.ndim != 2 or curves.shape[1] != self.n_in:
            raise ValueError("curves must be [B, %d], got %s" % (self.n_in, curves.shape))
        acc = numpy.zeros((len(curves), self.nx))
        lens, start = self._lens, self.rowptr[:-1]
        with numpy.errstate(all="ignore"):
            for l in range(int(lens.max()) if self.nx else 0):
                inside = l < lens
                p = numpy.where(inside, start + l, 0)                    # (a row that has ended: any entry, its product is dropped)
                acc = acc + numpy.where(inside[None, :], self.vals[p][None, :] * curves[:, self.cols[p]], 0.0)
        return acc[0] if one else acc

    def dense(self):
        """The matrix as ``R[nx, n_in]`` (absent entries 0)."""
        R = numpy.zeros((self.nx, self.n_in))
        R[numpy.repeat(numpy.arange(self.nx), self._lens), self.cols] = self.vals
        return R

    def bind(self):
        """The response on the GPU: a :class:`DeviceResponse` (close it, or drop it)."""
        return DeviceResponse(self)

    @classmethod
    def from_dense(cls, R, x_in=None):
        """``R[nx, n_in]`` -> the response of its entries that are not exactly zero."""
        R = numpy.asarray(R, dtype=float)
        if R.ndim != 2 or R.shape[0] < 1 or R.shape[1] < 1:
            raise ValueError("R must be [nx, n_in], got shape %s" % (R.shape,))
        keep = R != 0
        rowptr = numpy.concatenate(([0], numpy.cumsum(keep.sum(axis=1)))).astype(numpy.int64)
        rows, cols = numpy.nonzero(keep)                                   # (row-major: cols ascending inside a row)
        return cls(rowptr, cols.astype(numpy.int32), R[rows, cols], R.shape[1], x_in=x_in)

    @classmethod
    def from_ogip(cls, n_grp, f_chan, n_chan, matrix, n_channels, first_channel=0, arf=None, x_in=None):
        """The arrays of an RMF's MATRIX extension, per energy bin ``i`` of ``n_in = len(n_grp)``: ``n_grp[i]`` groups of
        consecutive channels, group ``g`` beginning at channel ``f_chan[i][g]`` (numbered from ``first_channel``, the
        extension's TLMIN of F_CHAN: 0 or 1) and ``n_chan[i][g]`` long, and ``matrix[i]``, the values of all groups one
        after the other.  ``f_chan[i]``, ``n_chan[i]`` and ``matrix[i]`` may be longer than what ``n_grp`` uses (fixed-
        width columns padded behind) and, where every bin has one group, scalars.  ``arf`` f64[n_in]: the effective area,
        multiplied into every value of its bin (one rounded product each).  Transposed to the channel-major CSR of
        :class:`Response`; entries that are exactly zero are kept as the file has them.  Pure numpy: no file is read."""
        n_grp = numpy.asarray(n_grp, dtype=numpy.int64)
        if n_grp.ndim != 1 or len(n_grp) < 1:
            raise ValueError("n_grp must be a one-dimensional array of n_in >= 1 entries, got shape %s" % (n_grp.shape,))
        n_in, n_channels = len(n_grp), int(n_channels)
        if len(f_chan) != n_in or len(n_chan) != n_in or len(matrix) != n_in:
            raise ValueError("f_chan, n_chan and matrix must have one entry per energy bin (%d)" % n_in)
        if arf is not None:
            arf = numpy.ascontiguousarray(arf, dtype=float)
            if arf.shape != (n_in,):
                raise ValueError("arf has shape %s, expected (%d,)" % (arf.shape, n_in))
        chans, bins, values = [], [], []
        for i in range(n_in):
            first = numpy.atleast_1d(numpy.asarray(f_chan[i], dtype=numpy.int64))
            count = numpy.atleast_1d(numpy.asarray(n_chan[i], dtype=numpy.int64))
            row = numpy.atleast_1d(numpy.asarray(matrix[i], dtype=float))
            G = int(n_grp[i])
            if G < 0 or G > len(first) or G > len(count):
                raise ValueError("n_grp[%d] = %d, f_chan[%d] and n_chan[%d] hold %d and %d groups" % (i, G, i, i, len(first), len(count)))
            at = 0
            for g in range(G):
                lo, n = int(first[g]) - int(first_channel), int(count[g])
                if n < 0 or lo < 0 or lo + n > n_channels:
                    raise ValueError("f_chan[%d][%d] = %d, n_chan[%d][%d] = %d: outside the %d channels from %d"
                                     % (i, g, first[g], i, g, n, n_channels, first_channel))
                if at + n > len(row):
                    raise ValueError("matrix[%d] holds %d values, its groups ask for %d at least" % (i, len(row), at + n))
                chans.append(numpy.arange(lo, lo + n))
                bins.append(numpy.full(n, i, dtype=numpy.int64))
                values.append(row[at:at + n] * arf[i] if arf is not None else row[at:at + n])
                at += n
        chans = numpy.concatenate(chans) if chans else numpy.zeros(0, dtype=numpy.int64)
        bins = numpy.concatenate(bins) if bins else numpy.zeros(0, dtype=numpy.int64)
        values = numpy.concatenate(values) if values else numpy.zeros(0)
        order = numpy.lexsort((bins, chans))                              # by channel, the bins ascending inside one
        chans, bins, values = chans[order], bins[order], values[order]
        twice = numpy.flatnonzero((chans[1:] == chans[:-1]) & (bins[1:] == bins[:-1]))
        if len(twice):
            k = int(twice[0])
            raise ValueError("matrix[%d]: two groups of the bin hold channel %d" % (bins[k], chans[k] + int(first_channel)))
        rowptr = numpy.concatenate(([0], numpy.cumsum(numpy.bincount(chans, minlength=n_channels)))).astype(numpy.int64)
        return cls(rowptr, bins.astype(numpy.int32), values, n_in, x_in=x_in)


class DeviceResponse(object):
    """A :class:`Response` resident on the device (``mdns_response_create``).  ``handle`` goes to
    ``mdns_spectra_set_response``; :meth:`fold` folds host curves through the device."""

    def __init__(self, response):
        self._lib = _lib.require_device()
        self._h = self._lib.mdns_response_create(response.nx, response.n_in, _lib.ptr(response.rowptr), _lib.ptr(response.cols),
                                                 _lib.ptr(response.vals))
        if not self._h:
            raise _lib.MdnsError("mdns_response_create failed: " + _lib.last_error())
        self.response, self.nx, self.n_in = response, response.nx, response.n_in

    @property
    def handle(self):
        if not self._h:
            raise _lib.MdnsError("the response was closed")
        return self._h

    def fold(self, curves):
        """``curves[B, n_in] -> folded[B, nx]`` on the device (mdns_response_fold_batch)."""
        curves = numpy.atleast_2d(_lib.as_f64(curves))
        if curves.shape[1] != self.n_in:
            raise ValueError("curves must be [B, %d], got %s" % (self.n_in, curves.shape))
        out = numpy.empty((len(curves), self.nx))
        _lib.check(self._lib.mdns_response_fold_batch(self.handle, _lib.ptr(curves), len(curves), _lib.ptr(out)), "mdns_response_fold_batch")
        return out

    def close(self):
        """Frees the device copy; refused (MdnsError) while a spectra handle still uses it."""
        if getattr(self, "_h", None):
            _lib.check(self._lib.mdns_response_destroy(self._h), "mdns_response_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ['Response', 'DeviceResponse']
