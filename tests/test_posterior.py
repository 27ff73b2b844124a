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


# ---- batches, edges and exact quantile ties: against the longdouble statement of posterior_support.py ------------
# (its derived bounds, its quantile classes -- the inputs have no slivers, so every quantile must be equal -- and
# numpy's draws, none of which lies within the clearance of a cdf boundary; test_posterior_host.py checks both
# conditions, the statement and the bounds without a device)

import posterior_support as ps


def _ids(cases):
    return [c[0] for c in cases]


@pytest.fixture(autouse=True)
def _default_scratch(monkeypatch):
    monkeypatch.delenv(ps.SCRATCH_VARIABLE, raising=False)


@pytest.mark.parametrize("case", ps.sweep_cases(), ids=_ids(ps.sweep_cases()))
def test_sweep_matches_statement(case):
    """Every nsamp around 64, 128, 256, kQLds and the longer slices, every ndata around the 64-lane groups and the
    256-thread combines, every ndim: within the derived bounds, and within the fixed ones of the first tests."""
    w, L, x, q, st = ps.stated(case)
    got = run_summary(w, L, x, q)
    ps.check_against_statement(got, st)
    check_summary(got, ref_summary(w, L, x, q), x, w, L, q)


@pytest.mark.parametrize("case", ps.quantile_cases(), ids=_ids(ps.quantile_cases()))
def test_quantile_cases_match_statement(case):
    """Dyadic ties (no allowance), key columns that exercise every level of the radix select, silent rows, rows
    placed at the ends, nq = 1 and 64: staged in LDS and read from the scratch."""
    w, L, x, q, st = ps.stated(case)
    ps.check_against_statement(run_summary(w, L, x, q), st)


def test_refusals():
    from massivedatans_amd._lib import MdnsError
    from massivedatans_amd.posterior import Posterior
    w = np.zeros((4, 2))
    with pytest.raises(MdnsError, match=r"ndim=9; 1 <= ndim <= 8"):
        Posterior(w, w, np.zeros((4, 2, ps.K_POST_DIM + 1)))
    with pytest.raises(MdnsError, match=r"ndim=0; 1 <= ndim <= 8"):
        Posterior(w, w, np.zeros((4, 2, 0)))
    x = np.arange(24.0).reshape(4, 2, 3)
    with Posterior(w, w, x) as post:
        for bad in ([0.0], [-0.25], [1.0 + 2.0 ** -52], [np.nan], [0.5, 1e-300, -0.0]):
            with pytest.raises(MdnsError, match=r"q\[%d\]=.* outside \(0, 1\]" % (len(bad) - 1)):
                post.summary(bad)
        with pytest.raises(MdnsError, match=r"nq=65 \(1\.\.64 quantiles\)"):
            post.summary(np.linspace(0.01, 0.99, ps.K_MAXQ + 1))
        with pytest.raises(MdnsError, match=r"n=0"):
            post.resample(0)
        got = post.summary(np.linspace(0.01, 0.99, ps.K_MAXQ))           # and the handle still answers
    ps.check_against_statement(got, ps.statement(w, w, x, got['q']))


def _batched(monkeypatch, per, b, call):
    monkeypatch.setenv(ps.SCRATCH_VARIABLE, str(b * per))
    try:
        return call()
    finally:
        monkeypatch.delenv(ps.SCRATCH_VARIABLE)


@pytest.mark.parametrize("case", ps.batch_cases(), ids=_ids(ps.batch_cases()))
def test_batches_equal_the_whole(case, monkeypatch):
    """Batches of 1, 64, 65, all but one and all data sets -- for the summary and for the resampling, whose bytes
    per data set differ -- give the bytes of the unbatched call, which is within the statement."""
    from massivedatans_amd.posterior import Posterior
    w, L, x, q, st = ps.stated(case)
    nsamp, ndata, ndim = x.shape
    n, seed, col = ps.BATCH_DRAWS
    with Posterior(w, L, x) as post:
        s0 = post.summary(q)
        r0, x0 = post.resample(n, seed=seed, gather=True, first_column=col)
    ps.check_against_statement(s0, st)
    ps.check_draws(r0, x0, w, L, x, seed, col)
    for b in ps.batch_sizes(ndata):
        with Posterior(w, L, x) as post:                                 # a fresh handle: its moments run again too
            s = _batched(monkeypatch, ps.summary_bytes(nsamp, ndim), b, lambda: post.summary(q))
            r, xd = _batched(monkeypatch, ps.resample_bytes(nsamp), b,
                             lambda: post.resample(n, seed=seed, gather=True, first_column=col))
        for k in ('nfinite', 'log_norm', 'ess', 'mean', 'std', 'quant', 'imaxL'):
            assert s[k].tobytes() == s0[k].tobytes(), (b, k)
        assert r.tobytes() == r0.tobytes() and xd.tobytes() == x0.tobytes(), b


def test_part_equals_whole_across_a_batch_boundary(monkeypatch):
    """test_part_equals_whole with batches of 64 in the whole and of 25 in the part [40, 100): a boundary of either
    falls inside the part."""
    from massivedatans_amd.posterior import Posterior
    w, L, x, q, _ = ps.stated(ps.batch_cases()[0])
    nsamp, ndata, ndim = x.shape
    lo, hi = 40, 100
    with Posterior(w, L, x) as whole:
        s = _batched(monkeypatch, ps.summary_bytes(nsamp, ndim), 64, lambda: whole.summary(Q))
        r = _batched(monkeypatch, ps.resample_bytes(nsamp), 64, lambda: whole.resample(100, seed=2))
    with Posterior(w[:, lo:hi], L[:, lo:hi], x[:, lo:hi]) as part:
        sp = _batched(monkeypatch, ps.summary_bytes(nsamp, ndim), 25, lambda: part.summary(Q))
        rp = _batched(monkeypatch, ps.resample_bytes(nsamp), 25, lambda: part.resample(100, seed=2, first_column=lo))
    for k in ('nfinite', 'log_norm', 'ess', 'mean', 'std', 'quant', 'imaxL'):
        assert s[k][lo:hi].tobytes() == sp[k].tobytes(), k
    assert r[lo:hi].tobytes() == rp.tobytes()


def test_deterministic_bytes_under_batches(monkeypatch):
    from massivedatans_amd.posterior import Posterior
    w, L, x, q, _ = ps.stated(ps.batch_cases()[0])
    nsamp, ndata, ndim = x.shape
    with Posterior(w, L, x) as a, Posterior(w, L, x) as b:
        s1, s2 = (_batched(monkeypatch, ps.summary_bytes(nsamp, ndim), 7, lambda: h.summary(Q)) for h in (a, b))
        r1, r2 = (_batched(monkeypatch, ps.resample_bytes(nsamp), 7, lambda: h.resample(500, seed=7)) for h in (a, b))
        s3 = _batched(monkeypatch, ps.summary_bytes(nsamp, ndim), 7, lambda: a.summary(Q))
    for k in s1:
        assert s1[k].tobytes() == s2[k].tobytes() == s3[k].tobytes(), k
    assert r1.tobytes() == r2.tobytes()


def _check_resample(w, L, x, calls):
    from massivedatans_amd.posterior import Posterior
    with Posterior(w, L, x) as post:
        for n, seed, col in calls:
            index, xd = post.resample(n, seed=seed, gather=True, first_column=col)
            ps.check_draws(index, xd, w, L, x, seed, col)
            plain = post.resample(n, seed=seed, first_column=col)
            assert plain.tobytes() == index.tobytes(), (n, seed, col)


@pytest.mark.parametrize("nsamp", ps.RESAMPLE_NSAMP)
def test_resample_sweep(nsamp):
    """n = 1, 2, 3, 5, 255, 257, 4001 (the tail of the last Philox block cut at every length) at nsamp below, at
    and above the 256 per-thread runs: every draw a finite row, gathered rows equal x[index], equal to numpy."""
    w, L, x = ps.resample_input(nsamp)
    _check_resample(w, L, x, ps.resample_calls(nsamp))


def test_resample_keys():
    """Every seed (0, 2^32, 2^63 + 5, 2^64 - 1) with every first column (0, 100, 2^40)."""
    w, L, x = ps.resample_input(257)
    _check_resample(w, L, x, ps.key_calls())


@pytest.mark.parametrize("nsamp", ps.PLACEMENT_NSAMP)
def test_resample_placements(nsamp):
    """Finite rows only in the last slice, only row 0, only the last row, none in the first and last 300 rows."""
    w, L, x = ps.placement_input(nsamp)
    _check_resample(w, L, x, [(257, 2 ** 63 + 5, 100), (4001, 0, 2 ** 40)])
