"""Posterior summaries and resampling on the GPU (mdns.h Part 7) against their numpy statement:
lw = w + L, F = rows where lw is finite, p = exp(lw[F] - max) / sum, the exact weighted moments, the
weighted quantiles of the sorted values, and Generator(Philox(key=[seed, d])).choice(F, n, p=p)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = (0.16, 0.5, 0.84, 0.025, 1.0)


# ---- the numpy statement ---------------------------------------------------------------------------------

def ref_summary(w, L, x, q):
    nsamp, ndata, ndim = x.shape
    q = np.asarray(q, float)
    out = dict(nfinite=np.zeros(ndata, int), log_norm=np.full(ndata, np.nan), ess=np.full(ndata, np.nan),
               mean=np.full((ndata, ndim), np.nan), std=np.full((ndata, ndim), np.nan),
               quant=np.full((ndata, ndim, len(q)), np.nan), imaxL=np.full(ndata, -1))
    for d in range(ndata):
        lw = w[:, d] + L[:, d]
        F = np.where(np.isfinite(lw))[0]
        out['nfinite'][d] = len(F)
        if len(F) == 0:
            continue
        m = lw[F].max()
        e = np.exp(lw[F] - m)
        S = e.sum()
        p = e / S
        out['log_norm'][d] = m + np.log(S)
        out['ess'][d] = 1.0 / (p ** 2).sum()
        xs = x[F, d, :]
        mean = p @ xs
        out['mean'][d] = mean
        out['std'][d] = np.sqrt(p @ (xs - mean) ** 2)
        for k in range(ndim):
            v = xs[:, k]
            o = np.argsort(v, kind='stable')
            c = np.cumsum(p[o])
            out['quant'][d, k] = v[o][np.minimum(np.searchsorted(c, q * c[-1], 'left'), len(v) - 1)]
        out['imaxL'][d] = F[np.argmax(L[F, d])]
    return out


def ref_weights(w, L, d):
    lw = w[:, d] + L[:, d]
    F = np.where(np.isfinite(lw))[0]
    if len(F) == 0:
        return F, None
    e = np.exp(lw[F] - lw[F].max())
    return F, e / e.sum()


def ref_choice(w, L, d, seed, n):
    """numpy's draws, and for each the distance of its uniform to the nearest cdf boundary."""
    F, p = ref_weights(w, L, d)
    if p is None:
        return np.full(n, -1), np.full(n, np.inf)
    idx = np.random.Generator(np.random.Philox(key=[seed, d])).choice(F, size=n, p=p)
    u = np.random.Generator(np.random.Philox(key=[seed, d])).random(n)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    j = np.searchsorted(cdf, u, 'right')
    near = np.minimum(np.abs(u - cdf[np.minimum(j, len(F) - 1)]), np.abs(u - cdf[np.maximum(j - 1, 0)]))
    return idx, near


# ---- inputs --------------------------------------------------------------------------------------------

def make(nsamp, ndata, ndim, seed=0, special=True):
    """Weights like a nested-sampling run (log widths falling, likelihoods rising), with the awkward
    columns in front: all -inf, one finite row, -inf holes, tied x, lw spread over 10^3, |mean|/std = 10^6."""
    rng = np.random.default_rng(seed)
    i = np.arange(nsamp)[:, None]
    w = -(i + 1.0) / 50.0 + rng.normal(0, 0.01, size=(nsamp, ndata))
    L = -0.5 * rng.chisquare(3, size=(nsamp, ndata)) * 20.0 * np.exp(-i / (nsamp / 5.0 + 1.0))
    x = rng.normal(size=(nsamp, ndata, ndim)) * rng.uniform(0.1, 10, size=(1, ndata, ndim)) \
        + rng.uniform(-5, 5, size=(1, ndata, ndim))
    holes = rng.uniform(size=(nsamp, ndata)) < 0.1
    w[holes] = -np.inf
    if special and ndata >= 6:
        w[:, 0] = -np.inf                                        # nothing finite
        w[:, 1] = -np.inf
        w[nsamp // 2, 1] = -1.0                                  # one finite row
        L[::2, 2] = -np.inf                                      # every other row lost
        x[:, 3, :] = np.round(x[:, 3, :])                       # tied values
        w[:, 4] = 0.0
        L[:, 4] = rng.uniform(-1000, 0, size=nsamp)             # most weights underflow
        x[:, 5, :] = 1e6 + rng.normal(size=(nsamp, ndim))        # |mean| / std = 10^6
        L[nsamp - 1, 6 % ndata] = np.nan                         # NaN is not finite either
    return w, L, x


def check_summary(got, want, x, w, L, q):
    assert np.array_equal(got['nfinite'], want['nfinite'])
    assert np.array_equal(got['imaxL'], want['imaxL'])
    ok = want['nfinite'] > 0
    assert np.all(np.isnan(got['log_norm'][~ok])) and np.all(np.isnan(got['mean'][~ok]))
    assert np.all(np.isnan(got['quant'][~ok]))

    def rel(a, b, scale):
        return np.max(np.abs(a - b) / scale) if a.size else 0.0

    assert rel(got['log_norm'][ok], want['log_norm'][ok], np.maximum(np.abs(want['log_norm'][ok]), 1.0)) <= 1e-12
    assert rel(got['ess'][ok], want['ess'][ok], want['ess'][ok]) <= 1e-12
    # mean relative to the weighted mean of |x| (a mean near zero has no relative digits of its own)
    scale = np.zeros_like(want['mean'])
    for d in np.where(ok)[0]:
        F, p = ref_weights(w, L, d)
        scale[d] = p @ np.abs(x[F, d, :])
    scale = np.maximum(scale, 1e-300)
    assert rel(got['mean'][ok], want['mean'][ok], scale[ok]) <= 1e-12
    sd = want['std'][ok]
    assert np.all(np.abs(got['std'][ok] - sd) <= 1e-10 * sd)
    # quantiles: numpy's value, or a sample value whose cumulative weight brackets q
    for d, k, j in zip(*np.where(got['quant'] != want['quant'])):
        if not ok[d]:
            continue
        F, p = ref_weights(w, L, d)
        v = x[F, d, k]
        g = got['quant'][d, k, j]
        assert g in v, (d, k, j, g)
        assert p[v < g].sum() <= q[j] + 1e-10 and p[v <= g].sum() >= q[j] - 1e-10, (d, k, j)


def run_summary(w, L, x, q=Q):
    from massivedatans_amd.posterior import Posterior
    with Posterior(w, L, x) as post:
        return post.summary(q)


@pytest.mark.parametrize("nsamp,ndata,ndim", [
    (1, 1, 1), (1, 65, 3), (7, 63, 3), (7, 64, 5), (1651, 65, 3), (1651, 64, 1), (1651, 1, 5), (1651, 10000, 3),
    (50000, 7, 3)])
def test_summary_matches_numpy(nsamp, ndata, ndim):
    w, L, x = make(nsamp, ndata, ndim, seed=nsamp + ndata + ndim)
    got = run_summary(w, L, x)
    check_summary(got, ref_summary(w, L, x, Q), x, w, L, Q)


def test_high_offset_std():
    w, L, x = make(1651, 8, 3, seed=5, special=False)
    x[:] = 600.0 + 0.01 * x / np.abs(x).max()                   # mu ~ 600 with a width ~ 0.01
    x[:, 1, :] = 1e6 + np.random.default_rng(1).normal(size=(1651, 3))
    got, want = run_summary(w, L, x), ref_summary(w, L, x, Q)
    assert np.max(np.abs(got['std'] - want['std']) / want['std']) <= 1e-10
    check_summary(got, want, x, w, L, Q)


@pytest.mark.parametrize("nsamp,ndata", [(7, 65), (1651, 64), (1651, 1000), (50000, 3)])
def test_resample_matches_numpy_choice(nsamp, ndata):
    from massivedatans_amd.posterior import Posterior
    w, L, x = make(nsamp, ndata, 3, seed=11)
    n, seed = 4000, 12345
    with Posterior(w, L, x) as post:
        index, xd = post.resample(n, seed=seed, gather=True)
    near_boundary = 0
    for d in range(ndata):
        want, near = ref_choice(w, L, d, seed, n)
        diff = index[d] != want
        assert np.all(near[diff] < 1e-12), (d, np.where(diff)[0][:5])
        near_boundary += int(diff.sum())
        if want[0] >= 0:
            assert np.array_equal(xd[d], x[index[d], d, :])
        else:
            assert np.all(np.isnan(xd[d]))
    assert near_boundary == 0


def test_deterministic_bytes():
    from massivedatans_amd.posterior import Posterior
    w, L, x = make(1651, 1000, 3, seed=3)
    with Posterior(w, L, x) as a, Posterior(w, L, x) as b:
        s1, s2 = a.summary(Q), b.summary(Q)
        r1, r2 = a.resample(500, seed=7), b.resample(500, seed=7)
        s3 = a.summary(Q)
    for k in s1:
        assert s1[k].tobytes() == s2[k].tobytes() == s3[k].tobytes(), k
    assert r1.tobytes() == r2.tobytes()


def test_part_equals_whole():
    """Columns summarised alone give the same bytes as inside the whole set (the .cols merge relies on it)."""
    from massivedatans_amd.posterior import Posterior
    w, L, x = make(1651, 300, 3, seed=4)
    with Posterior(w, L, x) as whole:
        s, r = whole.summary(Q), whole.resample(100, seed=2)
    with Posterior(w[:, 100:170], L[:, 100:170], x[:, 100:170]) as part:
        sp, rp = part.summary(Q), part.resample(100, seed=2, first_column=100)
    for k in ('nfinite', 'log_norm', 'ess', 'mean', 'std', 'quant', 'imaxL'):
        assert s[k][100:170].tobytes() == sp[k].tobytes(), k
    assert r[100:170].tobytes() == rp.tobytes()


def test_real_run_and_cli(tmp_path):
    """sample.run on gen.horns(100), summarised on the GPU and in numpy; then the CLI on the saved output,
    whole and as two .cols parts."""
    from massivedatans_amd import gen, sample
    from massivedatans_amd.posterior import summarize_results, weights_arrays
    d = gen.horns(100)
    results, sampler, _, duration = sample.run(d['x'], d['y'], nlive_points=100, use_graph=True, max_samples=3000)
    got = summarize_results(results, quantiles=Q, resample=1000, seed=3)
    w, L, x = weights_arrays(results['weights'])
    check_summary(got, ref_summary(w, L, x, Q), x, w, L, Q)
    for k in range(100):
        want, near = ref_choice(w, L, k, 3, 1000)
        assert np.all((got['index'][k] == want) | (near < 1e-12))
    assert np.array_equal(got['logZ'], results['logZ'])

    prefix = str(tmp_path / "run")
    gen.write_datasets(prefix + ".npz", dict(logZ=results['logZ'], logZerr=results['logZerr'], w=w, L=L, x=x))
    for lo, hi in ((0, 37), (37, 100)):
        gen.write_datasets("%s.cols%d-%d.npz" % (prefix, lo, hi), dict(
            logZ=results['logZ'][lo:hi], logZerr=results['logZerr'][lo:hi], w=w[:, lo:hi], L=L[:, lo:hi], x=x[:, lo:hi]))

    def cli(*args):
        out = subprocess.run([sys.executable, "-m", "massivedatans_amd.postprocess", *args, "--resample", "200", "--seed", "9"],
                             cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout

    text = cli(prefix + ".npz")
    assert "param 1" in text
    cli(prefix + ".cols37-100.npz", prefix + ".cols0-37.npz", "-o", prefix + ".merged.posterior.npz")
    with np.load(prefix + ".posterior.npz") as a, np.load(prefix + ".merged.posterior.npz") as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert np.array_equal(a['logZ'], results['logZ'])
        assert np.array_equal(a['quant'], got['quant'][:, :, :3])          # the CLI's default quantiles: Q[:3]
