"""The instrument response on the GPU (csrc/mdns_response.hip k_response_fold, include/mdns.h Part 13): the kernel
bit-equal to ``Response.statement`` at the edges of its workgroup, of its candidates per thread and of its layout,
non-finite bins, batches of changing size on one handle, draws and initial points under every curve statistic through a
spectra handle with the response against a response-less handle fed the statement's folded curves, ``background_fit``,
a whole run, and the handles' lifecycle and refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import GaussLineSpectra
from massivedatans_amd.response import DeviceResponse, Response
from curves_support import Chunks, dev_batch, gauss_prior, refused
from filter_support import _drive
from response_support import (N_IN, NDATA, NX, STATS, bins_and_channels, dev_fold, draw_response, lsf_response, make_spectra,
                              positive_model, random_response, stress_response, to_params)
from table_support import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_response_fold: 256 channels per workgroup, 64 per group of the layout, 4 candidates per thread
NXS = (1, 63, 64, 65, 255, 256, 257, 513)
N_INS = (1, 2, 300)
BS = (1, 2, 3, 4, 5, 7, 8, 9, 33)


@pytest.mark.parametrize("nx", NXS)
def test_kernel_equals_the_statement(nx, hip):
    """Both fold entries, every n_in and B, row strides with 0 and 3 doubles of padding: NaN behind the input rows, the
    output padding untouched."""
    for n_in in N_INS:
        rng = np.random.RandomState(1000 * nx + n_in)
        resp, planted = stress_response(rng, nx, n_in)
        if nx == 513:
            assert {"empty first", "empty last", "empty group", "one entry", "full row", "wave length 0", "wave length 1",
                    "wave length %d" % min(17, n_in), "wave length %d" % n_in, "negative"} <= set(planted)
        dr = resp.bind()
        assert hip.mdns_response_nx(dr.handle) == nx and hip.mdns_response_nin(dr.handle) == n_in
        for B in BS:
            curves = rng.normal(size=(B, n_in))
            want = resp.statement(curves)
            got = dr.fold(curves)
            assert got.shape == (B, nx) and same_bits(got, want), (n_in, B)
            empty = np.diff(resp.rowptr) == 0
            assert not np.signbit(got[:, empty]).any()
            for pad in (0, 3):
                wide, untouched = dev_fold(hip, dr, curves, pad, pad)
                assert same_bits(wide, want) and untouched, (n_in, B, pad)
        dr.close()


def test_a_banded_response_and_a_value_that_is_the_candidates_own(hip):
    """A line-spread function of the bench's kind; the same bits alone, at several places of a batch and in a permuted
    batch."""
    resp = lsf_response(300, 330, 3.0)
    rng = np.random.RandomState(2)
    curves = rng.uniform(size=(70, 330))
    dr = resp.bind()
    whole = dr.fold(curves)
    assert same_bits(whole, resp.statement(curves))
    alone = dr.fold(curves[17])
    assert same_bits(alone[0], whole[17])
    for place in (0, 3, 4, 69):
        batch = curves.copy()
        batch[place] = curves[17]
        assert same_bits(dr.fold(batch)[place], alone[0]) and same_bits(dev_fold(hip, dr, batch, 5, 2)[0][place], alone[0]), place
    perm = rng.permutation(70)
    assert same_bits(dr.fold(curves[perm]), whole[perm])
    dr.close()


def test_a_nan_and_an_inf_reach_the_channels_that_hold_the_bin():
    rng = np.random.RandomState(3)
    resp = random_response(rng, 130, 50, most=12)
    dr = resp.bind()
    curves = rng.normal(size=(6, 50))
    clean = dr.fold(curves)
    for value in (np.nan, np.inf, -np.inf):
        bad = curves.copy()
        where = [(1, 7), (4, 49), (5, 0)]                                  # (candidate, bin)
        for b, k in where:
            bad[b, k] = value
        got = dr.fold(bad)
        with np.errstate(all="ignore"):
            assert same_bits(got, resp.statement(bad))
        holds = resp.dense() != 0                                          # [nx, n_in] (random_response has no explicit zero)
        turned = ~np.isfinite(got)
        expect = np.zeros_like(turned)
        for b, k in where:
            expect[b] |= holds[:, k]
        assert np.array_equal(turned, expect) and expect.any()
        assert same_bits(got[~expect], clean[~expect])                     # no other channel, no other candidate
    dr.close()


def test_batches_of_changing_size_on_one_handle(hip):
    """33, 1 and 33 candidates through the handle's grow-only scratch, and through the folded buffer of a spectra handle:
    nothing stale is read."""
    rng = np.random.RandomState(4)
    resp = lsf_response(NX, N_IN, 2.0)
    dr = resp.bind()
    x, _ = bins_and_channels()
    y = rng.normal(size=(NX, 20))
    with_r, without = GaussLineSpectra(x, y, noise_level=0.5), GaussLineSpectra(x, y, noise_level=0.5)
    with_r.set_response(dr)
    assert with_r.n_in == N_IN and without.n_in == NX and with_r.response is dr
    for B in (33, 1, 33):
        curves = rng.normal(size=(B, N_IN))
        folded = resp.statement(curves)
        assert same_bits(dr.fold(curves), folded)
        assert np.array_equal(with_r.loglike_batch_curves(curves), without.loglike_batch_curves(folded))
        rows = np.array([3, 4, 17], dtype=np.int32)
        a = dev_batch(hip, with_r, curves, 3, rows, "mdns_curve_loglike_batch_dev", extra=(0.5,))
        b = dev_batch(hip, without, folded, 3, rows, "mdns_curve_loglike_batch_dev", extra=(0.5,))
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        with_r.loglike_batch_curves(np.zeros((2, NX)))                     # folded curves are not what these spectra take
    with_r.close()
    without.close()
    dr.close()


# ---- draws and initial points under every curve statistic ----
def _states(stat, route, nlive, calls):
    """``(dev, ref, closers)``: a state on spectra WITH the response whose model returns ``n_in`` bins (``route``: numpy
    curves, or a table bound to ``x_in``), and one on response-less spectra fed ``R.statement`` of the same curves."""
    tm, resp = positive_model(), draw_response()
    x, x_in = bins_and_channels()
    with_r, without = make_spectra(stat, tm, resp), make_spectra(stat, tm, resp)
    with_r.set_response(resp)

    def unfolded(xs):
        calls.append(len(xs))
        with np.errstate(all="ignore"):
            return tm.statement(x_in, xs)

    def folded(xs):
        with np.errstate(all="ignore"):
            return resp.statement(tm.statement(x_in, xs))
    table = None
    if route == "table":
        table = tm.bind(x_in)
        dev = jointstate.CurveJointState(with_r, nlive, lambda xs: pytest.fail("the table state called a model"), shelf_cap=4, table=table)
    else:
        dev = jointstate.CurveJointState(with_r, nlive, unfolded, shelf_cap=4, ndim=tm.ndim)
    ref = jointstate.CurveJointState(without, nlive, folded, shelf_cap=4, ndim=tm.ndim)
    assert dev.n_in == N_IN and dev.nx == NX and ref.n_in == NX
    return tm, dev, ref, [dev, ref] + ([table] if table else []) + [with_r, without]


@pytest.mark.parametrize("route", ["numpy", "table"])
@pytest.mark.parametrize("stat", STATS)
def test_draws_equal_draws_of_the_folded_curves(stat, route):
    """Live matrix after init -- with jitter under the table route --, then prepare / draw / advance rounds with random row
    selections and a cut-down: accepted index, fill bits, thresholds, shelf sizes and live matrix, to the bit.  Under the
    table route no curve is made in Python."""
    nlive, calls = 12, []
    tm, dev, ref, closers = _states(stat, route, nlive, calls)
    noisy = route == "table"
    rng = np.random.RandomState(len(stat) + 7 * noisy)
    convert = to_params(tm)
    xs0 = convert(gauss_prior(rng.uniform(size=(nlive, 3))))
    noise0 = rng.normal(0, 1e-5, size=(nlive, NDATA)) if noisy else None
    dev.init(xs0, jitter=noise0)
    ref.init(xs0, jitter=noise0)
    assert np.array_equal(dev.live_matrix(), ref.live_matrix()) and np.isfinite(dev.live_matrix()).all()
    ndraws = _drive(Chunks(dev, convert, noisy), Chunks(ref, convert, noisy), NDATA, rng, iterations=4, exact=True)
    assert ndraws > 0 and (len(calls) > ndraws if route == "numpy" else calls == [])
    for h in closers:
        h.close()


_TENSOR_SCRIPT = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch                                  # first: one HIP runtime per process
torch.cuda.set_device(0)
import numpy as np
from massivedatans_amd import jointstate
from curves_support import Chunks, gauss_prior
from filter_support import _drive
from response_support import N_IN, NDATA, NX, STATS, bins_and_channels, draw_response, make_spectra, positive_model, to_params
tm, resp = positive_model(), draw_response()
x, x_in = bins_and_channels()
convert = to_params(tm)
total = 0
for stat in STATS:
    with_r, without = make_spectra(stat, tm, resp), make_spectra(stat, tm, resp)
    with_r.set_response(resp)
    calls = []
    def as_tensor(xs):
        # rows of n_in + 5 doubles on the device, NaN behind the bins: read by pointer and row stride
        wide = torch.full((len(xs), N_IN + 5), float("nan"), dtype=torch.float64, device="cuda")
        with np.errstate(all="ignore"):
            wide[:, :N_IN] = torch.from_numpy(tm.statement(x_in, xs)).to("cuda")
        calls.append(len(xs))
        return wide[:, :N_IN]
    def folded(xs):
        with np.errstate(all="ignore"):
            return resp.statement(tm.statement(x_in, xs))
    dev = jointstate.CurveJointState(with_r, 12, as_tensor, shelf_cap=4, ndim=tm.ndim)
    ref = jointstate.CurveJointState(without, 12, folded, shelf_cap=4, ndim=tm.ndim)
    rng = np.random.RandomState(len(stat))
    xs0 = convert(gauss_prior(rng.uniform(size=(12, 3))))
    dev.init(xs0); ref.init(xs0)
    assert np.array_equal(dev.live_matrix(), ref.live_matrix())
    ndraws = _drive(Chunks(dev, convert, True), Chunks(ref, convert, True), NDATA, rng, iterations=3, exact=True)
    assert ndraws > 0 and len(calls) > ndraws
    total += ndraws
    # a tensor of nx columns is not what a state on these spectra takes
    dev.model = lambda xs: torch.zeros((len(xs), NX), dtype=torch.float64, device="cuda")
    try:
        dev.draw_params(xs0[:3], None)
        raise SystemExit("a tensor of nx columns was taken")
    except ValueError as e:
        assert "[3, %d]" % N_IN in str(e), e
    for h in (dev, ref, with_r, without):
        h.close()
print("TENSOR OK", total)
'''


def test_draws_from_a_device_tensor_of_n_in_columns(tmp_path):
    """``mdns_backend_draw_curves_dev`` under every statistic, the model a torch tensor on the device with padded rows.
    In a process of its own, torch imported first: the process must have one HIP runtime, and torch brings its own."""
    pytest.importorskip("torch")
    script = tmp_path / "response_tensor.py"
    script.write_text(_TENSOR_SCRIPT)
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MDNS_DEVICE="0"))
    assert out.returncode == 0 and "TENSOR OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


def test_scoring_outside_a_draw_takes_unfolded_curves(hip):
    """``loglike_batch_curves`` of every statistic, the continuum fit and ``background_fit``, host and device entries:
    spectra with the response given ``curves`` against response-less spectra given ``R.statement(curves)``."""
    tm, resp = positive_model(), draw_response()
    x, x_in = bins_and_channels()
    rng = np.random.RandomState(6)
    xs = to_params(tm)(gauss_prior(rng.uniform(size=(9, 3))))
    curves = tm.statement(x_in, xs)
    folded = resp.statement(curves)
    dr = resp.bind()
    mask = rng.uniform(size=NDATA) < 0.6
    rows = np.flatnonzero(mask).astype(np.int32)
    entry = dict(noise=("mdns_curve_loglike_batch_dev", (0.5,)), chi2=("mdns_curve_chi2_batch_dev", ()),
                 poisson=("mdns_curve_poisson_batch_dev", ()), wstat=("mdns_curve_wstat_batch_dev", ()))
    for stat in STATS:
        with_r, without = make_spectra(stat, tm, resp), make_spectra(stat, tm, resp)
        with_r.set_response(dr)
        score = "loglike_batch_curves" if hasattr(with_r, "loglike_batch_curves") else "loglike_batch"
        for m in (None, mask):
            a, b = getattr(with_r, score)(curves, m), getattr(without, score)(folded, m)
            assert np.array_equal(a, b) and np.isfinite(a).all(), (stat, m is None)
        if stat in entry:
            fn, extra = entry[stat]
            assert np.array_equal(dev_batch(hip, with_r, curves, 3, rows, fn, extra=extra), dev_batch(hip, without, folded, 3, rows, fn, extra=extra)), stat
        if stat == "continuum":
            for a, b in zip(with_r.continuum_fit(curves, mask), without.continuum_fit(folded, mask)):
                assert np.array_equal(a, b)
        if stat == "wstat":
            f = with_r.background_fit(curves, mask)
            assert f.shape == (9, len(rows), NX) and np.array_equal(f, without.background_fit(folded, mask))
            per = dev_batch(hip, with_r, curves, 3, rows, "mdns_curve_background_batch_dev", per=NX)
            assert np.array_equal(per, f)
        with_r.close()
        without.close()
    dr.close()


def test_whole_run_equals_the_run_on_folded_curves():
    """64 spectra, 100 live points, a table model bound to ``x_in`` and a numpy model: identical to the response-less run
    whose model folds by the statement."""
    tm, resp = positive_model(), draw_response()
    x, x_in = bins_and_channels()
    rng = np.random.RandomState(11)
    lo = np.array([tm.axes[0][0], tm.axes[1][0], 0.0, 0.5])
    hi = np.array([tm.axes[0][-1], tm.axes[1][-1], 0.2, 5.0])
    prior = lambda us: lo + (hi - lo) * np.asarray(us, dtype=float)
    truth = prior(rng.uniform(0.2, 0.8, size=(64, 4)))
    e = rng.uniform(0.5, 2.0, size=(NX, 64))
    y = rng.poisson(resp.statement(tm.statement(x_in, truth)).T * e * 20.0).astype(float)
    e = e * 20.0
    called = []

    def plain(xs):
        called.append(len(xs))
        with np.errstate(all="ignore"):
            return tm.statement(x_in, xs)

    def folding(xs):
        with np.errstate(all="ignore"):
            return resp.statement(tm.statement(x_in, xs))
    runs = []
    for model, response in ((tm, resp), (plain, resp), (folding, None)):
        p = problem.CurveProblem(x, y, model, prior, tm.ndim, poisson=True, exposure=e, response=response)
        assert (p.table is not None) == (model is tm) and (p.backend.response is not None) == (response is not None)
        if model is tm:
            assert p.table.nx == N_IN
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=100, max_samples=60, use_graph=False, seed=1)
        assert type(sampler.joint).__name__ == "CurveJointState"
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
        if response is not None:
            # outside a draw the problem takes parameters, its backend unfolded curves
            L = p.multi_loglikelihood_batch(truth[:5], np.ones(64, dtype=bool))
            assert np.array_equal(L, p.backend.loglike_batch_curves(tm.statement(x_in, truth[:5])))
        sampler.joint.close()
        p.backend.close()
    assert called and runs[0][2] > 0 and np.isfinite(runs[0][0]).all()
    for other in (1, 2):
        assert runs[0][2] == runs[other][2]
        for k in (0, 1, 3):
            assert np.array_equal(runs[0][k], runs[other][k]), (other, k)
    with pytest.raises(ValueError, match="x_in"):
        problem.CurveProblem(x, y, tm, prior, tm.ndim, poisson=True, exposure=e, response=lsf_response(NX, N_IN, 2.0))


# ---- lifecycle and refusals ----
def _raw_create(hip, nx, n_in, rowptr, cols, vals):
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    vals = np.ascontiguousarray(vals, dtype=float)
    return hip.mdns_response_create(nx, n_in, _lib.ptr(rowptr), _lib.ptr(cols), _lib.ptr(vals))


def test_refused_creates_name_the_array_and_the_index(hip):
    _lib.require_device()
    ok = dict(nx=3, n_in=3, rowptr=[0, 2, 2, 3], cols=[0, 2, 1], vals=[1.0, -2.0, 0.5])
    h = _raw_create(hip, **ok)
    assert h and hip.mdns_response_destroy(h) == 0
    cases = [
        (dict(nx=0), ("nx=0",)),
        (dict(nx=(1 << 20) + 1), ("nx=1048577",)),
        (dict(n_in=0), ("n_in=0",)),
        (dict(rowptr=[1, 2, 2, 3]), ("rowptr[0] = 1",)),
        (dict(rowptr=[0, 2, 1, 3]), ("rowptr[2] = 1 < rowptr[1] = 2",)),
        (dict(rowptr=[0, 2, 2, 1 << 31]), ("rowptr[3] = 2147483648", "2147483647 entries at most")),
        (dict(cols=[0, 3, 1]), ("cols[1] = 3 outside [0, 3)", "channel 0")),
        (dict(cols=[0, -1, 1]), ("cols[1] = -1 outside [0, 3)",)),
        (dict(cols=[2, 0, 1]), ("cols[1] = 0 after 2", "strictly increasing")),
        (dict(cols=[1, 1, 1]), ("cols[1] = 1 after 1",)),
        (dict(vals=[1.0, np.nan, 0.5]), ("vals[1] = nan is not finite",)),
        (dict(vals=[1.0, 2.0, np.inf]), ("vals[2] = inf is not finite", "channel 2")),
    ]
    for change, words in cases:
        assert not _raw_create(hip, **dict(ok, **change)), change
        msg = _lib.last_error()
        assert "mdns_response_create" in msg and all(w in msg for w in words), (msg, words)
    rp = np.array([0, 1], dtype=np.int64)
    assert not hip.mdns_response_create(1, 1, None, None, None) and "null rowptr" in _lib.last_error()
    assert not hip.mdns_response_create(1, 1, _lib.ptr(rp), None, None) and "null cols" in _lib.last_error()
    # the Python class refuses the same before any device call
    with pytest.raises(ValueError, match="cols\\[1\\] = 3 outside"):
        Response([0, 2, 2, 3], [0, 3, 1], [1.0, -2.0, 0.5], 3)
    # a matrix of no entries at all folds to +0.0
    empty = Response([0, 0, 0], [], [], 4).bind()
    got = empty.fold(np.full((3, 4), np.nan))
    assert (got == 0).all() and not np.signbit(got).any()
    empty.close()
    assert hip.mdns_response_destroy(None) == 0 and hip.mdns_response_nx(None) == -1 and hip.mdns_response_nin(None) == -1


def test_lifecycle_and_refusals(hip):
    tm, resp = positive_model(), draw_response()
    x, x_in = bins_and_channels()
    spectra = make_spectra("noise", tm, resp)
    plain = make_spectra("noise", tm, resp)
    dr = resp.bind()
    rng = np.random.RandomState(8)
    curves = rng.uniform(size=(8, N_IN))
    folded = resp.statement(curves)
    out = np.empty((8, NX))
    # the fold entries
    refused(hip.mdns_response_fold_batch(None, _lib.ptr(curves), 8, _lib.ptr(out)), "mdns_response_fold_batch", "null response")
    refused(hip.mdns_response_fold_batch(dr.handle, _lib.ptr(curves), -1, _lib.ptr(out)), "mdns_response_fold_batch", "B=-1")
    refused(hip.mdns_response_fold_batch(dr.handle, None, 8, _lib.ptr(out)), "mdns_response_fold_batch", "null argument")
    assert hip.mdns_response_fold_batch(dr.handle, None, 0, None) == 0
    d_c, d_o = hip.mdns_dev_alloc(curves.nbytes), hip.mdns_dev_alloc(out.nbytes)
    refused(hip.mdns_response_fold_batch_dev(dr.handle, d_c, N_IN - 1, 8, d_o, NX), "mdns_response_fold_batch_dev", "ldc=%d" % (N_IN - 1), "n_in=%d" % N_IN)
    refused(hip.mdns_response_fold_batch_dev(dr.handle, d_c, N_IN, 8, d_o, NX - 1), "mdns_response_fold_batch_dev", "ldo=%d" % (NX - 1), "nx=%d" % NX)
    assert hip.mdns_response_fold_batch_dev(dr.handle, d_c, N_IN, 0, d_o, NX) == 0
    with pytest.raises(ValueError):
        dr.fold(curves[:, :-1])
    # a response of another nx
    other = lsf_response(NX - 1, N_IN, 2.0).bind()
    refused(hip.mdns_spectra_set_response(spectra.handle, other.handle), "mdns_spectra_set_response", "%d channels" % (NX - 1), "have %d" % NX)
    with pytest.raises(_lib.MdnsError):
        spectra.set_response(other)
    assert spectra.response is None and spectra.n_in == NX
    refused(hip.mdns_spectra_set_response(None, dr.handle), "mdns_spectra_set_response", "null spectra")
    other.close()
    # attached: destroy is refused and frees nothing; the handles go on
    spectra.set_response(dr)
    refused(hip.mdns_response_destroy(dr.handle), "mdns_response_destroy", "attached to 1 spectra handle")
    with pytest.raises(_lib.MdnsError):
        dr.close()
    assert same_bits(dr.fold(curves), folded)
    want = plain.loglike_batch_curves(folded)
    assert np.array_equal(spectra.loglike_batch_curves(curves), want)
    # rows shorter than the response's bins
    L = hip.mdns_dev_alloc(8 * NDATA * 8)
    refused(hip.mdns_curve_loglike_batch_dev(spectra.handle, d_c, N_IN - 1, 8, 0.5, None, NDATA, L), "mdns_curve_loglike_batch_dev",
            "ldc=%d" % (N_IN - 1), "n_in=%d" % N_IN)
    # a table whose nx is not n_in, and one that fits; re-attaching under a live joint state
    wrong, right = tm.bind(x), tm.bind(x_in)
    js = jointstate.CurveJointState(spectra, 8, None, table=right)
    xs = to_params(tm)(gauss_prior(rng.uniform(size=(8, 3))))
    refused(hip.mdns_joint_init_table(js._h, wrong.handle, _lib.ptr(xs), 0.5, None), "mdns_joint_init_table", "%d bins" % NX, "takes %d" % N_IN)
    refused(hip.mdns_spectra_set_response(spectra.handle, None), "mdns_spectra_set_response", "a joint state exists")
    refused(hip.mdns_spectra_set_response(spectra.handle, dr.handle), "mdns_spectra_set_response", "a joint state exists")
    js.init(xs)
    live = js.live_matrix()
    js.prepare()
    acc, nsc = C.c_int(7), C.c_int(0)
    bits = np.zeros((NDATA + 63) // 64, dtype=np.uint64)
    outs = (C.addressof(acc), _lib.ptr(bits), C.addressof(nsc))
    _lib.check(hip.mdns_backend_draw_begin(js._h, None, NDATA), "mdns_backend_draw_begin")
    refused(hip.mdns_backend_draw_table(js._h, wrong.handle, _lib.ptr(xs), 8, None, *outs), "mdns_backend_draw_table", "%d bins" % NX)
    refused(hip.mdns_backend_draw_curves_dev(js._h, d_c, N_IN - 1, 8, None, *outs), "mdns_backend_draw_curves_dev", "%d bins" % N_IN)
    assert np.array_equal(js.live_matrix(), live)                          # nothing of it touched the state
    idx, _, beats, n = js.draw_params(to_params(tm)(gauss_prior(rng.uniform(size=(200, 3)) * [0.05, 1, 1])), None)
    assert n == 200 and idx >= 0 and beats.any()
    js.close()
    # detach, then destroy; a closed DeviceResponse says so; the spectra take channels again
    spectra.set_response(None)
    assert spectra.response is None and np.array_equal(spectra.loglike_batch_curves(folded), want)
    dr.close()
    dr.close()                                                             # (twice: nothing happens)
    with pytest.raises(_lib.MdnsError, match="closed"):
        dr.fold(curves)
    with pytest.raises(_lib.MdnsError, match="closed"):
        spectra.set_response(dr)
    # destroying the spectra releases a response they borrowed
    again = DeviceResponse(resp)
    spectra.set_response(again)
    spectra.close()
    again.close()
    for p in (d_c, d_o, L):
        hip.mdns_dev_free(p)
    for h in (wrong, right, plain):
        h.close()
