"""Test helpers of the posterior summaries (csrc/mdns_posterior.hip, mdns.h Part 7; test_posterior.py and
test_posterior_host.py): a plain statement of every output in ``np.longdouble``, the bounds the device's double
results must keep to it, an emulation of the kernels' own order of operations in numpy float64 (it checks the
statement and the bounds without a GPU), the classes of outcome a quantile may have, the input builders and
numpy's own draws.  Nothing here touches a device.

The statement, for log widths w and likelihoods L [nsamp][ndata] and parameters x [nsamp][ndata][ndim]:

    lw   = float64(w + L)             (the double sum is the definition)
    F    = rows where lw is finite,   m = max lw[F],   t_i = m - lw_i >= 0
    e_i  = exp(-t_i),  S = sum e,  p = e / S            (longdouble from here on)
    log_norm = m + log S,   ess = 1 / sum p^2,   mean_k = sum p x_k,   std_k = sqrt(sum p (x_k - mean_k)^2)
    imaxL = the first row of F with the largest L
    quantile q of parameter k = the smallest sample value v (in the order of the device's 64-bit key, which
          keeps -0.0 below +0.0) with  sum of W_i over rows with x_ik <= v  >=  q * sum W,   W_i = p_i 2^52

The bounds.  u = 2^-53.  The device sums a data set's rows slice by slice and then the slices in order
(mdns_posterior_create: rows_per_slice = max(128, ceil(nsamp / 64)), nslices = ceil(nsamp / rows_per_slice)), so
a sum of non-negative terms passes through at most R - 1 additions, R = rows_per_slice + nslices, and carries a
relative error of at most (R - 1) u to first order.  A device weight e_i is exp of the rounded difference
fl(lw_i - m) = -t_i (1 + d), |d| <= u, which moves exp by t_i u relatively, and exp itself is good to one ulp,
2 u: e_i is within (2 + t_i) u of the statement's.  A term e_i a_i whose a_i carries a relative error of a u and
whose product is rounded once is therefore within (3 + a + t_i) u, and

    | sum e a  (device)  -  sum e a | <= u [ (R + 2 + a) sum e |a|  +  sum e t |a| ]                        (*)

Everything below is (*) with the quantity's own scale; `tbar` = sum p t, `tbar2` = sum p^2 t / sum p^2.

    S         a = 1 (a = 0, no product):  relative eS = (R + 1 + tbar) u
    log_norm  log(S (1 + eS)) = log S + eS, log good to one ulp, one rounded addition:
              |d log_norm| <= u (R + 1 + tbar + 2 |log S| + |log_norm|)
    ess       S^2 / S2, S2 = sum e^2: a term e^2 is within (2 (2 + t_i) + 1) u, the sum adds (R - 1) u, then one
              product and one quotient:  relative <= (2 (R + 1 + tbar) + (R + 4 + 2 tbar2) + 2) u
    mean_k    sx_k / S with (*), a = 0, then the error of S and one quotient:
              |d mean_k| <= u [ (R + 2) A_k + T_k + (R + 2 + tbar) |mean_k| ],  A_k = sum p |x_k|, T_k = sum p t |x_k|
    std_k     the device's centred sum uses its own mean, mean + dm: sum p (x - mean - dm)^2 = var + dm^2 exactly.
              c = fl(x - mean') carries u, c c carries 2 u + u, e (c c) one more: a = 3 in (*) with the product;
              then / S and the square root, which halves the relative error and rounds once:
              th = u [ (R + 5) + TV_k / var_k + (R + 1 + tbar) + 1 ],  TV_k = sum p t (x_k - mean_k)^2
              |d std_k| <= std_k (th / 2 + u) + min(dm, dm^2 / (2 std_k)) (1 + th),  dm = the bound of the mean
              The last term is the second-order (dm / std)^2 std / 2; it is dm itself where std = 0.

Every bound is multiplied by (1 + 2^-20) for the terms of second order and has the statement's own error added:
a longdouble sum of nsamp terms is good to nsamp 2^-64 relatively (of the same scale).

The quantile classes, in fixed-point units (one unit = 2^-52 of the total weight).  The device selects on
W'_i = rint(e'_i / S' 2^52) and target = ceil(fl(q tot')), tot' = sum W' (an integer below 2^53, exact in a
double).  A cumulative integer sum C' >= ceil(y) exactly when C' >= y, so the ceiling costs nothing; the product
is rounded once (half a unit at most).  S' scales every weight and the total alike and drops out to first order.
What remains between C'_k - target and the statement's C_k - q 2^52 is: the rounding of rint, half a unit per row,
weighted (1 - q) before and q after the value, nsamp / 2 at most; the subtraction in the exponent,
2^52 u sum t_i e_i / S <= nsamp / (2 e) < 0.19 nsamp (t exp(-t) <= 1 / e, S >= 1); one ulp of exp over a total
weight of one, one unit; the
quotient, half a unit; the product, half a unit.  Together 0.69 nsamp + 2 <= slack = nsamp + 2.

    must    the target clears the cumulative sums on both sides of the answer by more than `slack`:
            the value is determined and the device must return it, bit for bit
    exact   the weights are dyadic by construction (lw equal on a power-of-two number of finite rows: e = 1,
            S = n, W = 2^52 / n and tot = 2^52 without any rounding): integer arithmetic gives the answer
            and there is no allowance at all
    sliver  anything else: every value whose cumulative sums bracket the target within `slack` passes

q = 1.0 asks for target = tot' and q < 2^-53 for target = 1 (the device floors it there): the answer is the largest
(smallest) value among the rows whose fixed-point weight is not zero, W_i > 1/2.  It is determined -- class must --
unless some row's W_i lies within 2^-20 of 1/2.

Outside the inputs built as ties there are no slivers at all; test_posterior_host.py asserts that for every input
the GPU tests use, so on the device every quantile must be equal."""
import fractions
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SECOND = 1.0 + 2.0 ** -20
FIX = 2 ** 52

# the constants of csrc/mdns_posterior.hip
K_POST_DIM = 8
K_QBLOCK = 256
K_QLDS = 3840
K_SLICE_ROWS = 128
K_MAXQ = 64
K_SCRATCH_BYTES = 512 << 20
SCRATCH_VARIABLE = "MDNS_POST_SCRATCH_BYTES"

MUST, EXACT, SLIVER = 0, 1, 2

#: the quantiles of the shape sweep: unsorted, with a duplicate, both ends
Q_SWEEP = (0.16, 0.5, 0.84, 0.025, 1.0, 1e-300, 0.5, 0.999)


def plan(nsamp):
    """What mdns_posterior_create and the kernels derive from nsamp."""
    rows = (nsamp + 63) // 64
    rps = rows if rows > K_SLICE_ROWS else K_SLICE_ROWS
    nslices = (nsamp + rps - 1) // rps
    return dict(rows_per_slice=rps, nslices=nslices, R=rps + nslices, staged=nsamp <= K_QLDS,
                chunk=(nsamp + K_QBLOCK - 1) // K_QBLOCK)


def summary_bytes(nsamp, ndim):
    """Scratch bytes of one data set in mdns_posterior_summary (transposed x and the fixed-point weights)."""
    return nsamp * (ndim + 1) * 8


def resample_bytes(nsamp):
    """Scratch bytes of one data set in mdns_posterior_resample (the cdf)."""
    return nsamp * 8


def batch_of(budget, per, ndata):
    """post_batch: data sets per launch under a scratch budget."""
    return min(ndata, max(1, budget // per))


def keys(v):
    """The device's order-preserving 64-bit key of a double (post_key)."""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def unkeys(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def _is_dyadic(lwF):
    n = len(lwF)
    return n > 0 and (n & (n - 1)) == 0 and bool(np.all(lwF == lwF[0]))


def _groups(kv, weight):
    """Distinct keys in ascending order and the cumulative weight up to and including each."""
    o = np.argsort(kv, kind='stable')
    ks = kv[o]
    first = np.concatenate(([True], ks[1:] != ks[:-1]))
    last = np.concatenate((first[1:], [True]))
    return ks[first], np.cumsum(weight[o])[last]


def _target_exact(q, tot):
    """ceil(q tot) as the device computes it where fl(q tot) is exact (tot a power of two), floored at 1."""
    t = fractions.Fraction(float(q)) * tot
    return min(tot, max(1, math.ceil(t)))


# ---------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------

def statement(w, L, x, q):
    """Every output of mdns_posterior_summary from the definitions, in np.longdouble, with the scales the bounds
    need and the class of every quantile.  `quant` holds the value the device must return (class must / exact)
    or the statement's own choice (class sliver)."""
    nsamp, ndata, ndim = x.shape
    q = np.asarray(q, float).reshape(-1)
    nq = len(q)
    slack = nsamp + 2
    nan = lambda *s: np.full(s, np.nan, LD)
    out = dict(nfinite=np.zeros(ndata, int), imaxL=np.full(ndata, -1), log_norm=nan(ndata), logS=nan(ndata),
               ess=nan(ndata), tbar=nan(ndata), tbar2=nan(ndata), mean=nan(ndata, ndim), std=nan(ndata, ndim),
               A=nan(ndata, ndim), T=nan(ndata, ndim), TV=nan(ndata, ndim),
               quant=np.full((ndata, ndim, nq), np.nan), qclass=np.full((ndata, ndim, nq), MUST),
               q=q, nsamp=nsamp, slack=slack, _inputs=(w, L, x))
    lw_all = np.asarray(w, np.float64) + np.asarray(L, np.float64)
    with np.errstate(all='ignore'):
        for d in range(ndata):
            lw = lw_all[:, d]
            F = np.where(np.isfinite(lw))[0]
            out['nfinite'][d] = len(F)
            if len(F) == 0:
                continue
            out['imaxL'][d] = F[np.argmax(L[F, d])]
            m = lw[F].max()
            t = LD(m) - lw[F].astype(LD)
            e = np.exp(-t)
            S = e.sum()
            p = e / S
            out['logS'][d] = np.log(S)
            out['log_norm'][d] = LD(m) + np.log(S)
            p2 = p * p
            out['ess'][d] = 1 / p2.sum()
            out['tbar'][d] = (p * t).sum()
            out['tbar2'][d] = (p2 * t).sum() / p2.sum()
            xs = x[F, d, :].astype(LD)
            mean = p @ xs
            c2 = (xs - mean) ** 2
            out['mean'][d] = mean
            # the device squares x - mean in double: the statement holds where that square is a double
            out['std'][d] = np.where(c2.max(axis=0) < LD(2.0) ** 1023, np.sqrt(p @ c2), LD(np.nan))
            out['A'][d] = p @ np.abs(xs)
            out['T'][d] = (p * t) @ np.abs(xs)
            out['TV'][d] = (p * t) @ c2
            dyadic = _is_dyadic(lw[F])
            W = p * LD(FIX)
            for k in range(ndim):
                kv = keys(x[F, d, k])
                if dyadic:
                    uk, C = _groups(kv, np.full(len(F), FIX // len(F), dtype=object))
                    for j in range(nq):
                        target = _target_exact(q[j], FIX)
                        out['quant'][d, k, j] = unkeys(uk[[next(i for i, c in enumerate(C) if c >= target)]])[0]
                        out['qclass'][d, k, j] = EXACT
                    continue
                uk, C = _groups(kv, W)
                for j in range(nq):
                    if q[j] == 1.0 or q[j] * 2.0 ** 53 < 1.0:
                        heard = W > 0.5
                        pick = kv[heard].max() if q[j] == 1.0 else kv[heard].min()
                        out['quant'][d, k, j] = unkeys(np.array([pick]))[0]
                        if np.any(np.abs(W - LD(0.5)) <= 2.0 ** -20):
                            out['qclass'][d, k, j] = SLIVER
                        continue
                    T = LD(q[j]) * LD(FIX)
                    i = min(int(np.searchsorted(C, T, 'left')), len(C) - 1)
                    out['quant'][d, k, j] = unkeys(uk[[i]])[0]
                    above = i == len(C) - 1 or C[i] - T > slack
                    below = i == 0 or T - C[i - 1] > slack
                    if not (above and below):
                        out['qclass'][d, k, j] = SLIVER
    return out


def bounds(st):
    """The derived bounds of the device's double results (see the module's docstring), as arrays."""
    R = plan(st['nsamp'])['R']
    own = st['nsamp'] * 2.0 ** -64                       # the statement's own longdouble sums
    with np.errstate(all='ignore'):
        tbar, tbar2 = st['tbar'].astype(float), st['tbar2'].astype(float)
        eS = (R + 1 + tbar) * U
        ln = np.abs(st['log_norm']).astype(float)
        log_norm = SECOND * U * (R + 1 + tbar + 2 * np.abs(st['logS']).astype(float) + ln) + own * np.maximum(ln, 1.0)
        ess = st['ess'].astype(float) * (SECOND * U * (2 * (R + 1 + tbar) + (R + 4 + 2 * tbar2) + 2) + 3 * own)
        A, T, mu = st['A'].astype(float), st['T'].astype(float), np.abs(st['mean']).astype(float)
        mean = SECOND * U * ((R + 2) * A + T + (R + 2 + tbar)[:, None] * mu) + 2 * own * A
        sd, TV = st['std'].astype(float), st['TV'].astype(float)
        th = U * ((R + 5) + np.where(sd > 0, TV / (sd * sd), 0.0) + (R + 1 + tbar)[:, None] + 1)
        second = np.where(sd > 0, np.minimum(mean, mean * mean / (2 * np.where(sd > 0, sd, 1.0))), mean)
        std = SECOND * (sd * (th / 2 + U) + second * (1 + th)) + 2 * own * sd
    return dict(log_norm=log_norm, ess=ess, mean=mean, std=std, eS=eS)


#: the largest error seen as a fraction of its bound, by quantity (a report, asserted nowhere)
SEEN = dict(log_norm=0.0, ess=0.0, mean=0.0, std=0.0)


def check_against_statement(got, st, moments=True, quantiles=True, seen=SEEN):
    """The outputs `got` (a device summary or the emulation) against the statement: counts and arg-max equal,
    moments within the derived bounds wherever the statement's value and its bound are finite, quantiles equal
    in the classes must and exact and bracketing in sliver."""
    assert np.array_equal(got['nfinite'], st['nfinite'])
    assert np.array_equal(got['imaxL'], st['imaxL'])
    none = st['nfinite'] == 0
    for name in ('log_norm', 'ess', 'mean', 'std', 'quant'):
        assert np.all(np.isnan(got[name][none])), name
    if moments:
        bd = bounds(st)
        for name in ('log_norm', 'ess', 'mean', 'std'):
            want = st[name]
            use = np.isfinite(want.astype(float)) & np.isfinite(bd[name])
            with np.errstate(all='ignore'):
                err = np.abs(got[name].astype(LD) - want).astype(float)
            assert np.all(np.isfinite(got[name][use])), name
            bad = use & ~(err <= bd[name])
            assert not bad.any(), (name, np.argwhere(bad)[:5].tolist(), err[bad][:5], bd[name][bad][:5])
            frac = err[use & (bd[name] > 0)] / bd[name][use & (bd[name] > 0)]
            if frac.size:
                seen[name] = max(seen[name], float(frac.max()))
    if quantiles and got['quant'].size:
        same = keys(got['quant']) == keys(st['quant'])
        same |= np.isnan(got['quant']) & np.isnan(st['quant'])
        firm = st['qclass'] != SLIVER
        bad = firm & ~same
        assert not bad.any(), ("quantile", np.argwhere(bad)[:5].tolist(), got['quant'][bad][:5], st['quant'][bad][:5])
        for d, k, j in np.argwhere(~firm & ~same):
            assert sliver_allows(st, d, k, j, got['quant'][d, k, j]), (d, k, j)


def sliver_allows(st, d, k, j, value):
    """A sliver's allowance: `value` is a sample value of a finite row whose cumulative weights bracket the target
    within the slack."""
    w, L, x = st['_inputs']
    lw = w[:, d] + L[:, d]
    F = np.where(np.isfinite(lw))[0]
    t = LD(lw[F].max()) - lw[F].astype(LD)
    e = np.exp(-t)
    W = e / e.sum() * LD(FIX)
    kv, kg = keys(x[F, d, k]), keys(np.array([value]))[0]
    if kg not in kv:
        return False
    T = LD(st['q'][j]) * LD(FIX)
    return W[kv < kg].sum() <= T + st['slack'] and W[kv <= kg].sum() >= T - st['slack']


# ---------------------------------------------------------------------------------------
# the kernels' own order, in numpy float64
# ---------------------------------------------------------------------------------------

def emulate(w, L, x, q):
    """mdns_posterior_summary in numpy float64 in the kernels' order: every data set's rows slice by slice, the
    slices in order, three passes (max, sums, centred second moment), then the fixed-point weights
    rint(p 2^52) as integers and an integer weighted select on the device's keys."""
    nsamp, ndata, ndim = x.shape
    q = np.asarray(q, float).reshape(-1)
    pl = plan(nsamp)
    rps, nsl = pl['rows_per_slice'], pl['nslices']
    w, L, x = np.asarray(w, np.float64), np.asarray(L, np.float64), np.asarray(x, np.float64)
    with np.errstate(all='ignore'):
        lw = w + L
        fin = np.isfinite(lw)
        m = np.where(fin, lw, -np.inf).max(axis=0)
        nfin = fin.sum(axis=0)
        imax = np.full(ndata, -1)
        for d in np.where(nfin > 0)[0]:
            F = np.where(fin[:, d])[0]
            imax[d] = F[np.argmax(L[F, d])]                         # the first row of the largest L within F
        e = np.where(fin, np.exp(lw - m), 0.0)
        xz = np.where(fin[:, :, None], x, 0.0)

        def sliced(term):
            """sum over rows of term [nsamp, ...]: sequentially within a slice, then the slices in order"""
            tot = np.zeros(term.shape[1:])
            for s in range(nsl):
                acc = np.zeros(term.shape[1:])
                for i in range(s * rps, min(nsamp, (s + 1) * rps)):
                    acc = acc + term[i]
                tot = tot + acc
            return tot

        se, se2 = sliced(e), sliced(e * e)
        sx = sliced(e[:, :, None] * xz)
        ok = nfin > 0
        log_norm = np.where(ok, m + np.log(se), np.nan)
        ess = np.where(ok, se * se / se2, np.nan)
        mean = np.where(ok[:, None], sx / se[:, None], np.nan)
        c = np.where(fin[:, :, None], x - mean, 0.0)
        sv = sliced(e[:, :, None] * (c * c))
        std = np.where(ok[:, None], np.sqrt(sv / se[:, None]), np.nan)
        quant = np.full((ndata, ndim, len(q)), np.nan)
        for d in np.where(ok)[0]:
            F = np.where(fin[:, d])[0]
            W = np.rint(e[F, d] / se[d] * float(FIX)).astype(np.int64)
            tot = int(W.sum())
            heard = W > 0
            for k in range(ndim):
                uk, C = _groups(keys(x[F[heard], d, k]), W[heard])
                for j in range(len(q)):
                    t = math.ceil(q[j] * float(tot))
                    target = 1 if t < 1 else min(tot, t)
                    quant[d, k, j] = unkeys(uk[[int(np.searchsorted(C, target, 'left'))]])[0]
    return dict(nfinite=nfin.astype(np.int32), imaxL=imax.astype(np.int32), log_norm=log_norm, ess=ess, mean=mean,
                std=std, quant=quant)


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------

def make(nsamp, ndata, ndim, seed=0, special=True):
    """test_posterior.make: weights like a nested-sampling run (log widths falling, likelihoods rising), with the
    awkward columns in front: all -inf, one finite row, -inf holes, tied x, lw spread over 10^3,
    |mean| / std = 10^6, a NaN."""
    rng = np.random.default_rng(seed)
    i = np.arange(nsamp)[:, None]
    w = -(i + 1.0) / 50.0 + rng.normal(0, 0.01, size=(nsamp, ndata))
    L = -0.5 * rng.chisquare(3, size=(nsamp, ndata)) * 20.0 * np.exp(-i / (nsamp / 5.0 + 1.0))
    x = rng.normal(size=(nsamp, ndata, ndim)) * rng.uniform(0.1, 10, size=(1, ndata, ndim)) \
        + rng.uniform(-5, 5, size=(1, ndata, ndim))
    holes = rng.uniform(size=(nsamp, ndata)) < 0.1
    w[holes] = -np.inf
    if special and ndata >= 6:
        w[:, 0] = -np.inf
        w[:, 1] = -np.inf
        w[nsamp // 2, 1] = -1.0
        L[::2, 2] = -np.inf
        x[:, 3, :] = np.round(x[:, 3, :])
        w[:, 4] = 0.0
        L[:, 4] = rng.uniform(-1000, 0, size=nsamp)
        x[:, 5, :] = 1e6 + rng.normal(size=(nsamp, ndim))
        L[nsamp - 1, 6 % ndata] = np.nan
    return w, L, x


#: (nsamp, ndata, ndim) of the sweep: every value of every axis, every ndim at a ragged (nsamp, ndata); ndata = 257
#: crosses the 256-thread combine kernels
SHAPES = ((1, 1, 1), (2, 63, 2), (63, 64, 3), (64, 65, 3), (65, 129, 4), (127, 65, 7), (128, 63, 6), (129, 65, 8),
          (255, 1, 8), (256, 64, 1), (257, 129, 6), (3839, 65, 1), (3840, 63, 3), (3841, 65, 5), (8191, 63, 7),
          (8192, 64, 6), (8193, 65, 8), (129, 257, 3), (8193, 1, 1))
NSAMP_AXIS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3839, 3840, 3841, 8191, 8192, 8193)
NDATA_AXIS = (1, 63, 64, 65, 129, 257)
#: the staged and the unstaged column of the quantile cases
QUANTILE_NSAMP = (3840, 3841)
#: the batched shapes
BATCH_SHAPES = ((257, 130, 3), (3841, 70, 3))


def sweep_input(shape):
    nsamp, ndata, ndim = shape
    return make(nsamp, ndata, ndim, seed=1000 + nsamp + ndata + ndim)


def batch_input(shape):
    nsamp, ndata, ndim = shape
    return make(nsamp, ndata, ndim, seed=2000 + nsamp)


def batch_sizes(ndata):
    """Data sets per batch the batched tests ask for: 1, 64, 65 (a short final batch at both shapes), one short of
    everything, and exactly everything."""
    return (1, 64, 65, ndata - 1, ndata)


def _rows(nsamp, n, place, rng):
    if place == 'first':
        return np.arange(n)
    if place == 'last':
        return np.arange(nsamp - n, nsamp)
    return np.sort(rng.choice(nsamp, n, replace=False))


def tie_counts(nsamp):
    """Finite rows of the dyadic columns: 4096 needs a column longer than any staged one."""
    return tuple(n for n in (1, 2, 64, 256, 4096) if n <= nsamp)


def tie_quantiles(n):
    """q = j / n exactly, j / n +- 2^-40, and the doubles next to j / n (there q 2^52 is no integer, so the
    ceiling in the target decides), for j at both ends and around the middle; at most 64."""
    js = sorted({j for j in (1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n) if 1 <= j <= n})
    q = []
    for j in js:
        c = j / n
        for v in (c, c + 2.0 ** -40, c - 2.0 ** -40, np.nextafter(c, 2.0), np.nextafter(c, 0.0)):
            if 0.0 < v <= 1.0:
                q.append(float(v))
    assert len(q) <= K_MAXQ
    return np.array(q)


def dyadic_input(nsamp, n, seed=7):
    """w = 0 and L constant on n = 2^k finite rows (the first rows, the last rows, scattered rows: one data set
    each), holes elsewhere: p = 1 / n and the fixed-point weights are exact.  Distinct x in the first parameter, x
    with ties in the second."""
    rng = np.random.default_rng(seed + n)
    w = np.full((nsamp, 3), -np.inf)
    L = np.full((nsamp, 3), -3.25)
    x = rng.normal(size=(nsamp, 3, 2))
    x[:, :, 1] = np.round(4 * x[:, :, 1])
    for d, place in enumerate(('first', 'last', 'scattered')):
        w[_rows(nsamp, n, place, rng), d] = 0.0
    return w, L, x


KEY_COLUMNS = ('negative', 'zeros', 'equal', 'last byte', 'magnitudes', 'infinite')
#: the quantiles of the key columns; with the 'infinite' column's weights the answers are -inf, finite, +inf in turn
Q_KEYS = (1e-300, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0)


def key_input(nsamp, seed=21):
    """One data set per key column (KEY_COLUMNS), two parameters (the column and its mirror image), weights of
    make() without its special columns."""
    rng = np.random.default_rng(seed)
    w, L, _ = make(nsamp, len(KEY_COLUMNS), 1, seed=seed, special=False)
    x = np.empty((nsamp, len(KEY_COLUMNS), 2))
    x[:, 0, 0] = -np.exp(rng.normal(size=nsamp) * 3)
    z = rng.normal(size=nsamp)
    z[rng.uniform(size=nsamp) < 0.3] = 0.0
    z[rng.uniform(size=nsamp) < 0.3] = -0.0
    x[:, 1, 0] = z
    x[:, 2, 0] = 2.5
    x[:, 3, 0] = 1.0 + rng.integers(0, 256, size=nsamp) * 2.0 ** -52
    mag = np.array([5e-324, 2.0 ** -1060, 2.2250738585072014e-308, 1e-200, 1e-100, 1e-30, 1e-5, 1.0, 3.0, 1e5, 1e30,
                    1e100, 1e200, 1e300])
    x[:, 4, 0] = rng.choice(np.concatenate((mag, -mag)), size=nsamp)
    x[:, 5, 0] = rng.normal(size=nsamp)
    # the infinite column: equal weights on the middle rows, 0.119 of the weight at each infinity (exp(2.5): no
    # cumulative weight meets a quantile of Q_KEYS)
    w[:, 5], L[:, 5] = -np.inf, 0.0
    mid = np.arange(nsamp // 2 - 40, nsamp // 2 + 41)        # 79 plain rows: the median is no tie
    w[mid, 5] = 0.0
    w[mid[3], 5] = w[mid[60], 5] = 2.5
    x[mid[3], 5, 0], x[mid[60], 5, 0] = np.inf, -np.inf
    x[:, :, 1] = -x[:, :, 0]
    return w, L, x


def silent_input(nsamp, seed=31):
    """w = 0, L in (-3, 0), and two rows of F with p < 2^-54 -- their fixed-point weight is zero -- that hold the
    column's largest and smallest value: q = 1.0 and q = 1e-300 must not answer with them.  Three data sets: the
    silent rows first and last, in the middle, and next to each other."""
    rng = np.random.default_rng(seed)
    w = np.zeros((nsamp, 3))
    L = rng.uniform(-3, 0, size=(nsamp, 3))
    x = rng.normal(size=(nsamp, 3, 2))
    for d, (a, b) in enumerate(((0, nsamp - 1), (nsamp // 2, nsamp // 3), (100, 101))):
        L[[a, b], d] = -40.0 - math.log(nsamp)
        x[a, d, :] = (50.0, -50.0)
        x[b, d, :] = (-60.0, 60.0)
    return w, L, x


Q_SILENT = (1.0, 1e-300, 0.5)

PLACEMENTS = ('last slice', 'row 0', 'last row', 'edges lost', 'plain')


def placement_input(nsamp, seed=41):
    """Finite rows only in the last slice, only row 0, only the last row, and none in the first and last 300 rows
    (where the cdf search meets flat runs at both ends and whole threads' runs are empty); the last data set is
    make()'s plain one."""
    w, L, x = make(nsamp, len(PLACEMENTS), 2, seed=seed, special=False)
    pl = plan(nsamp)
    w[:(pl['nslices'] - 1) * pl['rows_per_slice'], 0] = -np.inf
    w[nsamp - 1, 0] = -1.0
    w[:, 1] = -np.inf
    w[0, 1] = 0.5
    w[:, 2] = -np.inf
    w[nsamp - 1, 2] = 0.5
    w[:300, 3] = -np.inf
    w[nsamp - 300:, 3] = -np.inf
    w[nsamp // 2, 3] = -1.0
    return w, L, x


PLACEMENT_NSAMP = (700, 3841)

# ---------------------------------------------------------------------------------------
# resampling
# ---------------------------------------------------------------------------------------

N_AXIS = (1, 2, 3, 5, 255, 257, 4001)
SEED_AXIS = (0, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1)
COLUMN_AXIS = (0, 100, 2 ** 40)
#: nsamp of the resampling sweep: below, at and above the 256 per-thread runs, and a long column
RESAMPLE_NSAMP = (1, 2, 255, 256, 257, 3841)
RESAMPLE_NDATA = 7


def resample_input(nsamp):
    """make() with its special columns, and a second data set without finite rows behind a plain one: a draw
    stored one slot too far lands in a row that must read -1 throughout."""
    w, L, x = make(nsamp, RESAMPLE_NDATA, 2, seed=3000 + nsamp)
    w[:, 5] = -np.inf
    return w, L, x


def resample_calls(nsamp):
    """(n, seed, first_column) of the sweep at one nsamp: every n, the seeds and first columns in rotation."""
    at = RESAMPLE_NSAMP.index(nsamp)
    return [(n, SEED_AXIS[(i + at) % 4], COLUMN_AXIS[(i + at) % 3]) for i, n in enumerate(N_AXIS)]


def key_calls():
    """Every seed with every first column (n = 5, so the tail of the last Philox block is cut too)."""
    return [(5, s, c) for s in SEED_AXIS for c in COLUMN_AXIS]


#: (n, seed, first_column) of the draws in the batched tests
BATCH_DRAWS = (37, 2 ** 32, 100)


def clearance(nsamp):
    """Both cdfs are sums of at most nsamp non-negative terms that are one ulp of exp apart, divided by their last
    element: they differ by about 2 nsamp 2^-53 at most.  The factor 64 leaves a margin of about thirty."""
    return 64.0 * nsamp * 2.0 ** -53


def draws(w, L, d, seed, first_column, n):
    """numpy's Generator(Philox(key=[seed, first_column + d])).choice(F, n, p=p) and the distance of every draw's
    uniform to the nearest boundary of numpy's cdf; -1 and inf for a data set without finite rows."""
    lw = w[:, d] + L[:, d]
    F = np.where(np.isfinite(lw))[0]
    if len(F) == 0:
        return np.full(n, -1), np.full(n, np.inf)
    e = np.exp(lw[F] - lw[F].max())
    p = e / e.sum()
    key = np.array([int(seed), (int(first_column) + d) % 2 ** 64], dtype=np.uint64)
    idx = np.random.Generator(np.random.Philox(key=key)).choice(F, size=n, p=p)
    u = np.random.Generator(np.random.Philox(key=key)).random(n)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    j = np.searchsorted(cdf, u, 'right')
    assert np.array_equal(F[np.minimum(j, len(F) - 1)], idx)
    upper = cdf[np.minimum(j, len(F) - 1)]
    lower = np.where(j > 0, cdf[np.maximum(j - 1, 0)], -np.inf)     # below the first boundary there is only 0 <= u
    return idx, np.minimum(np.abs(u - upper), np.abs(u - lower))


def check_draws(index, xdraws, w, L, x, seed, first_column):
    """Device draws against numpy's: every index a finite row of its data set (or every one -1 where there is
    none), the gathered rows equal to x[index], and -- no reference draw lies within the clearance, asserted here
    and on the CPU tier -- equal to numpy's on every draw."""
    nsamp, ndata = w.shape
    n = index.shape[1]
    lw = w + L
    for d in range(ndata):
        fin = np.isfinite(lw[:, d])
        if not fin.any():
            assert np.all(index[d] == -1), d
            assert xdraws is None or np.all(np.isnan(xdraws[d])), d
            continue
        assert np.all((index[d] >= 0) & (index[d] < nsamp)), d
        assert np.all(fin[index[d]]), (d, "a draw outside F")
        if xdraws is not None:
            assert xdraws[d].tobytes() == np.ascontiguousarray(x[index[d], d, :]).tobytes(), d
        want, near = draws(w, L, d, seed, first_column, n)
        assert near.min() > clearance(nsamp), (d, "the reference draw is not determined: change the seed")
        assert np.array_equal(index[d], want), (d, np.where(index[d] != want)[0][:5])


# ---------------------------------------------------------------------------------------
# the cases both tiers run, and their statements (computed once per session)
# ---------------------------------------------------------------------------------------

def quantile_cases():
    """(name, builder of (w, L, x), q) of the built quantile inputs, each at a staged and an unstaged nsamp."""
    cases = []
    for nsamp in QUANTILE_NSAMP + (5000,):
        for n in tie_counts(nsamp):
            if nsamp == 5000 and n != 4096:
                continue                                   # 5000 is there for the one count no staged column holds
            cases.append(("ties-%d-%d" % (nsamp, n), lambda nsamp=nsamp, n=n: dyadic_input(nsamp, n), tie_quantiles(n)))
    for nsamp in QUANTILE_NSAMP:
        cases.append(("keys-%d" % nsamp, lambda nsamp=nsamp: key_input(nsamp), np.array(Q_KEYS)))
        cases.append(("silent-%d" % nsamp, lambda nsamp=nsamp: silent_input(nsamp), np.array(Q_SILENT)))
        cases.append(("nq1-%d" % nsamp, lambda nsamp=nsamp: make(nsamp, 7, 2, seed=51), np.array([0.3])))
        cases.append(("nq64-%d" % nsamp, lambda nsamp=nsamp: make(nsamp, 7, 2, seed=52),
                      np.random.default_rng(53).uniform(0.001, 0.999, size=K_MAXQ)))
    for nsamp in PLACEMENT_NSAMP:
        cases.append(("placement-%d" % nsamp, lambda nsamp=nsamp: placement_input(nsamp), np.array(Q_SWEEP)))
    return cases


def sweep_cases():
    return [("sweep-%d-%d-%d" % s, lambda s=s: sweep_input(s), np.array(Q_SWEEP)) for s in SHAPES]


def batch_cases():
    return [("batch-%d-%d-%d" % s, lambda s=s: batch_input(s), np.array(Q_SWEEP)) for s in BATCH_SHAPES]


def all_cases():
    return sweep_cases() + batch_cases() + quantile_cases()


_STATED = {}


def stated(case):
    """(w, L, x, q, statement) of a case; built once and left unchanged."""
    name, build, q = case
    if name not in _STATED:
        w, L, x = build()
        for a in (w, L, x):
            a.setflags(write=False)
        _STATED[name] = (w, L, x, q, statement(w, L, x, q))
    return _STATED[name]
