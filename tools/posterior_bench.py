"""Posterior summaries and resampling on the GPU (mdns.h Part 7) against the host loops they replace.

    python tools/posterior_bench.py [nsamp ndata ndim ndraws]      (default: 1651 10000 3 4000, the C2 shape)

Prints one JSON line: the upload, the device time of every phase (events inside the library), the bytes
the kernels must move by the model below and their rate against the HBM rate measured on the MI355X
(6.29 TB/s), and the host time of the numpy statement (exact moments + weighted quantiles + numpy's
choice, data set by data set) and of the reference-style loop (musefuse_postprocess.py:112-140:
normalise, choice of ndraws, mean and std of the draws) on the same arrays.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.29e12
Q = (0.16, 0.5, 0.84)


def make(nsamp, ndata, ndim, seed=0):
    rng = np.random.default_rng(seed)
    i = np.arange(nsamp)[:, None]
    w = -(i + 1.0) / 400.0 + rng.normal(0, 0.01, size=(nsamp, ndata))
    L = -0.5 * rng.chisquare(3, size=(nsamp, ndata)) * 20.0 * np.exp(-i / (nsamp / 5.0 + 1.0))
    x = rng.normal(size=(nsamp, ndata, ndim)) + rng.uniform(400, 800, size=(1, ndata, ndim))
    w[rng.uniform(size=(nsamp, ndata)) < 0.05] = -np.inf
    return w, L, x


def modelled_bytes(nsamp, ndata, ndim, nq, ndraws):
    """Bytes each phase has to move at least (8-byte doubles / integer weights, 4-byte indices)."""
    e, x = nsamp * ndata * 8, nsamp * ndata * ndim * 8
    return dict(
        moments=2 * e + (2 * e + x),                      # max pass (w, L); sums pass (w, L, x)
        std=2 * e + x,                                    # centred pass (w, L, x)
        quantiles=(2 * e + x) + 2 * (e + x) + (e + x),    # transpose: read w, L, x, write x and weights; select: read them
        resample=2 * e + 2 * e + ndata * ndraws * 4,      # cdf: read w, L, write and read the cdf; draws out
    )


def numpy_statement(w, L, x, ndraws, seed=1):
    nsamp, ndata, ndim = x.shape
    for d in range(ndata):
        lw = w[:, d] + L[:, d]
        F = np.where(np.isfinite(lw))[0]
        e = np.exp(lw[F] - lw[F].max())
        p = e / e.sum()
        xs = x[F, d, :]
        mean = p @ xs
        np.sqrt(p @ (xs - mean) ** 2)
        for k in range(ndim):
            v = xs[:, k]
            o = np.argsort(v, kind='stable')
            c = np.cumsum(p[o])
            v[o][np.minimum(np.searchsorted(c, np.asarray(Q) * c[-1]), len(v) - 1)]
        np.random.Generator(np.random.Philox(key=[seed, d])).choice(F, size=ndraws, p=p)


def reference_loop(w, L, x, ndraws):
    weights = np.transpose(w + L)
    points = np.swapaxes(x, 0, 1)
    for wd, xd in zip(weights, points):
        jparent = np.where(np.isfinite(wd))[0]
        wd = wd[jparent]
        wd = np.exp(wd - wd.max())
        wd = wd / wd.sum()
        j = np.random.choice(jparent, size=ndraws, p=wd)
        xequal = xd[j, :]
        for k in range(xd.shape[1]):
            xequal[:, k].mean()
            xequal[:, k].std()


def main(argv):
    nsamp, ndata, ndim, ndraws = (int(v) for v in (argv + [1651, 10000, 3, 4000][len(argv):]))
    from massivedatans_amd import _lib
    from massivedatans_amd.posterior import Posterior
    _lib.require_device()
    w, L, x = make(nsamp, ndata, ndim)
    with Posterior(w, L, x) as warm:                       # code objects loaded, allocator warm
        warm.summary(Q)
        warm.resample(ndraws, seed=1)
    t0 = time.perf_counter()
    post = Posterior(w, L, x)
    t_upload = time.perf_counter() - t0
    t0 = time.perf_counter()
    s = post.summary(Q)
    t_summary = time.perf_counter() - t0
    t0 = time.perf_counter()
    post.resample(ndraws, seed=1)
    t_resample = time.perf_counter() - t0
    ms = post.timings()
    post.close()
    model = modelled_bytes(nsamp, ndata, ndim, len(Q), ndraws)
    kernel_ms = sum(ms.values())
    total_bytes = sum(model.values())
    t0 = time.perf_counter()
    numpy_statement(w, L, x, ndraws)
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    reference_loop(w, L, x, ndraws)
    t_ref = time.perf_counter() - t0
    out = dict(
        shape=dict(nsamp=nsamp, ndata=ndata, ndim=ndim, ndraws=ndraws, nq=len(Q)),
        upload_s=t_upload, summary_call_s=t_summary, resample_call_s=t_resample,
        kernel_ms=ms, kernel_ms_total=kernel_ms,
        modelled_bytes=model, modelled_bytes_total=total_bytes,
        hbm_fraction={k: (model[k] / (ms[k] * 1e-3)) / HBM if ms[k] > 0 else None for k in model},
        hbm_fraction_total=(total_bytes / (kernel_ms * 1e-3)) / HBM if kernel_ms > 0 else None,
        host_numpy_statement_s=t_numpy, host_reference_loop_s=t_ref,
        finite_data_sets=int((s['nfinite'] > 0).sum()))
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
