"""The fixed-scale chi^2 with per-pixel variances on the GPU (csrc/mdns_curves.hip k_curve_rows_w, include/mdns.h
Part 9): the kernel against its numpy statement within the derived bound and against the emulated chain bit for bit,
the one value of a (curve, spectrum) pair, the exact reductions to the fixed-noise kernel, masked pixels as deleted
channels, the joint state and a whole run against their numpy statements over the same scores, and what is refused."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate, problem, sample
from massivedatans_amd.like import GaussLineSpectra, MuseSpectra, WeightedSpectra
from chi2_support import DeviceScorer, NumpyWeightedChi2, chain, rel_bound, weighted_data
from curves_support import (STAGE_EDGE_BS, STAGE_EDGE_CASES, STAGE_EDGE_NDATA, STAGE_EDGE_NX, Chunks, StatementProblem, dev_batch,
                            gauss_prior, line_model, refused, selections)
from filter_support import _drive

pytestmark = pytest.mark.gpu

NX, NDATA, BS = STAGE_EDGE_NX, STAGE_EDGE_NDATA, STAGE_EDGE_BS
CASES = STAGE_EDGE_CASES


def test_the_cases_cover_every_size():
    assert {c[0] for c in CASES} == set(NX) and {c[1] for c in CASES} == set(NDATA) and {c[2] for c in CASES} == set(BS)
    assert len(set(CASES)) == 30


@pytest.mark.parametrize("nx,ndata,B", CASES)
def test_kernel_against_the_statement(nx, ndata, B, hip):
    """Every L within (nx + 4) 2^-53 (relative) of the longdouble statement -- chi2_support derives the bound --, pairs
    whose statement is 0 equal to it, both entry points the same bits, and some pairs bit-equal to the emulated chain."""
    rng = np.random.RandomState(nx * 1000 + B)
    masked = (nx + ndata + B) % 2 == 0
    d = weighted_data(ndata, nx, seed=2, masked=masked)
    if masked and nx > 2:
        d["v"][:, ndata // 2] = np.inf                                       # one spectrum without a good pixel
    st = NumpyWeightedChi2(d["y"], d["v"])
    spectra = WeightedSpectra(d["x"], d["y"], d["v"])
    assert np.array_equal(spectra.n_masked, st.n_masked)
    curves = rng.uniform(-0.1, 0.3, size=(B, nx))
    want = st.loglike_batch_long(curves)
    worst = 0.0
    for name, rows in selections(ndata, rng):
        ref = want if rows is None else want[:, rows]
        got = spectra.loglike_batch_curves(curves, rows)
        assert got.shape == ref.shape
        zero = ref == 0
        assert np.array_equal(got[zero], np.zeros(int(zero.sum()))), name
        err = np.abs(got.astype(np.longdouble) - ref)[~zero] / np.abs(ref[~zero])
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert (err <= rel_bound(nx)).all(), (name, float(err.max()), rel_bound(nx))
        assert np.array_equal(dev_batch(hip, spectra, curves, 3, rows, "mdns_curve_chi2_batch_dev"), got), name
        assert np.array_equal(spectra.loglike_batch(curves, rows), got), name
    print("nx=%d ndata=%d B=%d masked=%s: max rel err %.3g (bound %.3g)" % (nx, ndata, B, masked, worst, rel_bound(nx)))
    whole = spectra.loglike_batch_curves(curves)
    for b, k in {(0, 0), (B - 1, ndata - 1), (B // 2, ndata // 2)}:
        assert whole[b, k] == chain(curves[b], st.y[:, k], st.w[:, k]), (b, k)
    spectra.close()


def test_a_pair_has_one_value(hip):
    """The same bits for (curve b, spectrum k) in a batch of 70 x 300, alone, in a permuted batch over a selection,
    through the device entry with another row stride, and in the live matrix of a joint state."""
    rng = np.random.RandomState(11)
    nx, ndata, B = 200, 300, 70
    d = weighted_data(ndata, nx, seed=4, masked=True)
    curves = rng.uniform(0, 0.2, size=(B, nx))
    spectra = WeightedSpectra(d["x"], d["y"], d["v"])
    whole = spectra.loglike_batch_curves(curves)
    for b, k in [(0, 0), (69, 299), (31, 63), (32, 64), (33, 127), (8, 128), (7, 256), (64, 129)]:
        alone = spectra.loglike_batch_curves(curves[b:b + 1], np.array([k]))
        assert alone.shape == (1, 1) and np.array_equal(alone[0, 0], whole[b, k]), (b, k)
    perm = rng.permutation(B)
    sel = np.sort(rng.choice(ndata, size=137, replace=False))
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm], sel), whole[perm][:, sel])
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm[:5]], sel[3:4]), whole[perm[:5]][:, sel[3:4]])
    for pad in (0, 1, 56):
        assert np.array_equal(dev_batch(hip, spectra, curves[perm], pad, sel, "mdns_curve_chi2_batch_dev"), whole[perm][:, sel]), pad
    nlive = 40
    js = jointstate.CurveJointState(spectra, nlive, lambda xs: curves[xs[:, 0].astype(int)])
    js.init(np.arange(20, 20 + nlive, dtype=float)[:, None])
    assert np.array_equal(js.live_matrix(), whole[20:20 + nlive])
    js.close()
    spectra.close()


@pytest.mark.parametrize("v,noise", [(1.0, 1.0), (0.25, 0.5)])
def test_exact_reduction_to_the_fixed_noise_kernel(v, noise):
    """A power-of-two weight commutes with every rounding: v = noise^2 everywhere gives the bits of
    mdns_curve_loglike_batch at that noise level."""
    nx, ndata, B = 65, 130, 33
    d = weighted_data(ndata, nx, seed=5)
    rng = np.random.RandomState(5)
    curves = rng.uniform(-0.1, 0.3, size=(B, nx))
    weighted = WeightedSpectra(d["x"], d["y"], np.full_like(d["y"], v))
    fixed = GaussLineSpectra(d["x"], d["y"], noise_level=noise)
    sel = np.arange(1, ndata, 2)
    for rows in (None, sel):
        assert np.array_equal(weighted.loglike_batch_curves(curves, rows), fixed.loglike_batch_curves(curves, rows))
    weighted.close()
    fixed.close()


@pytest.mark.parametrize("name,bad", [("first", [0]), ("last", [95]), ("stage", list(range(32, 64))), ("scattered", [1, 31, 32, 64, 94]),
                                      ("all but one", [j for j in range(96) if j != 40])])
def test_a_masked_pixel_is_a_deleted_channel(name, bad):
    """v = inf, y = NaN in some channels of every spectrum: the bits of the same data with those channels deleted."""
    nx, ndata, B = 96, 70, 9
    d = weighted_data(ndata, nx, seed=6)
    rng = np.random.RandomState(6)
    curves = rng.uniform(-0.1, 0.3, size=(B, nx))
    y, v = d["y"].copy(), d["v"].copy()
    y[bad] = np.nan
    v[bad] = np.inf
    keep = np.setdiff1d(np.arange(nx), bad)
    with_mask = WeightedSpectra(d["x"], y, v)
    deleted = WeightedSpectra(d["x"][keep], np.ascontiguousarray(d["y"][keep]), np.ascontiguousarray(d["v"][keep]))
    assert (with_mask.n_masked == len(bad)).all() and (deleted.n_masked == 0).all()
    a = with_mask.loglike_batch_curves(curves)
    b = deleted.loglike_batch_curves(np.ascontiguousarray(curves[:, keep]))
    assert np.array_equal(a, b) and (a < 0).all()
    with_mask.close()
    deleted.close()


def test_a_spectrum_without_a_good_pixel_scores_zero():
    nx, ndata, B = 96, 70, 9
    d = weighted_data(ndata, nx, seed=7)
    d["v"][:, 3] = np.inf
    d["y"][:, 64] = np.nan
    spectra = WeightedSpectra(d["x"], d["y"], d["v"])
    assert spectra.n_masked[3] == nx and spectra.n_masked[64] == nx and spectra.n_masked.sum() == 2 * nx
    L = spectra.loglike_batch_curves(np.random.RandomState(7).uniform(-0.1, 0.3, size=(B, nx)))
    assert (L[:, [3, 64]] == 0).all() and (np.delete(L, [3, 64], axis=1) < 0).all()
    spectra.close()


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("ndata,nlive,nx", [(20, 8, 64), (130, 12, 33)])
def test_joint_state_equals_its_numpy_statement(ndata, nlive, nx, noisy):
    """CurveJointState over WeightedSpectra against HostJointState fed by the same kernel: accepted index, fill bits,
    thresholds and live matrix equal, over several prepare / draw / advance rounds, with and without likelihood noise."""
    rng = np.random.RandomState(ndata * 7 + nlive + noisy)
    d = weighted_data(ndata, nx, seed=8, masked=True)
    spectra = WeightedSpectra(d["x"], d["y"], d["v"])
    model = line_model(d["x"])
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(DeviceScorer(spectra), nlive, ndata, model)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    noise0 = rng.normal(0, 1e-5, size=(nlive, ndata)) if noisy else None
    dev.init(xs0, jitter=noise0)
    host.init(xs0, jitter=noise0)
    assert dev.nparams == 3 and np.array_equal(dev.live_matrix(), host.live_matrix())
    want = NumpyWeightedChi2(d["y"], d["v"]).loglike_batch_long(model(xs0)).astype(float) + (noise0 if noisy else 0)
    assert np.allclose(dev.live_matrix(), want, rtol=1e-12, atol=0)
    assert _drive(Chunks(dev, lambda xs: xs, noisy), Chunks(host, model, noisy), ndata, rng, iterations=8, exact=True) > 0
    dev.close()
    spectra.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_whole_run_equals_the_statement(use_graph):
    d = weighted_data(12, 160, seed=9, masked=True)
    x, y, v = d["x"][96:160], np.ascontiguousarray(d["y"][96:160]), np.ascontiguousarray(d["v"][96:160])
    model = line_model(x)
    runs = []
    for cls in (problem.CurveProblem, StatementProblem):
        p = cls(x, y, model, gauss_prior, 3, v=v, marginalise_scale=False)
        assert isinstance(p.backend, WeightedSpectra)
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=20, max_samples=40, use_graph=use_graph, seed=1)
        assert type(sampler.joint).__name__ == ("CurveJointState" if cls is problem.CurveProblem else "HostJointState")
        assert sampler.native is not None
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert runs[0][2] > 0 and runs[0][2] == runs[1][2]
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_the_mode_is_set_only_where_it_has_a_meaning(hip):
    d = weighted_data(20, 64, seed=10)
    plain = GaussLineSpectra(d["x"], d["y"], noise_level=0.01)
    refused(hip.mdns_spectra_set_fixed_scale(plain.handle, 1), "mdns_spectra_set_fixed_scale", "without variances")
    assert hip.mdns_spectra_fixed_scale(plain.handle) == 0 and hip.mdns_spectra_fixed_scale(None) == -1
    curves = np.zeros((2, 64))
    out = np.zeros((2, 20))
    refused(hip.mdns_curve_chi2_batch(plain.handle, _lib.ptr(curves), 2, None, 20, _lib.ptr(out)), "spectra were created without variances")
    plain.close()
    # a handle in either mode scores the same through the pure batch call
    muse = MuseSpectra(d["x"], d["y"], d["v"])
    weighted = WeightedSpectra(d["x"], d["y"], d["v"])
    assert hip.mdns_spectra_fixed_scale(muse.handle) == 0 and hip.mdns_spectra_fixed_scale(weighted.handle) == 1
    curves = np.random.RandomState(1).uniform(-0.1, 0.3, size=(5, 64))
    got = np.empty((5, 20))
    assert hip.mdns_curve_chi2_batch(muse.handle, _lib.ptr(curves), 5, None, 20, _lib.ptr(got)) == 0
    assert np.array_equal(got, weighted.loglike_batch_curves(curves))
    # ... and the scale-marginalised batch call computes what its name says in either mode
    marg = np.empty((5, 20))
    assert hip.mdns_muse_loglike_batch(weighted.handle, _lib.ptr(curves), 5, None, 20, _lib.ptr(marg)) == 0
    assert np.array_equal(marg, muse.loglike_batch(curves))
    # a continuum excludes the mode, and the mode a continuum
    assert hip.mdns_spectra_set_continuum(muse.handle, 2) == 0
    refused(hip.mdns_spectra_set_fixed_scale(muse.handle, 1), "mdns_spectra_set_fixed_scale", "continuum")
    assert hip.mdns_spectra_fixed_scale(muse.handle) == 0 and hip.mdns_spectra_continuum(muse.handle) == 2
    assert hip.mdns_spectra_set_continuum(muse.handle, 0) == 0
    refused(hip.mdns_spectra_set_continuum(weighted.handle, 2), "mdns_spectra_set_continuum", "fixed-scale")
    assert hip.mdns_spectra_continuum(weighted.handle) == 0 and hip.mdns_spectra_fixed_scale(weighted.handle) == 1
    # fixed while a joint state lives on the handle, in both directions
    for sp, now in ((muse, 0), (weighted, 1)):
        js = jointstate.CurveJointState(sp, 8, line_model(d["x"]))
        refused(hip.mdns_spectra_set_fixed_scale(sp.handle, 1 - now), "mdns_spectra_set_fixed_scale", "a joint state exists")
        assert hip.mdns_spectra_fixed_scale(sp.handle) == now
        js.close()
    assert hip.mdns_spectra_set_fixed_scale(muse.handle, 1) == 0 and hip.mdns_spectra_fixed_scale(muse.handle) == 1
    assert hip.mdns_spectra_set_fixed_scale(muse.handle, 0) == 0 and hip.mdns_spectra_fixed_scale(muse.handle) == 0
    # sizes
    refused(hip.mdns_curve_chi2_batch(weighted.handle, _lib.ptr(curves), 5, None, 21, _lib.ptr(got)), "mdns_curve_chi2_batch", "M=21")
    d_c = hip.mdns_dev_alloc(curves.nbytes)
    d_o = hip.mdns_dev_alloc(got.nbytes)
    refused(hip.mdns_curve_chi2_batch_dev(weighted.handle, d_c, 63, 5, None, 20, d_o), "mdns_curve_chi2_batch_dev", "ldc=63", "nx=64")
    assert hip.mdns_curve_chi2_batch_dev(weighted.handle, d_c, 64, 0, None, 20, d_o) == 0
    assert hip.mdns_curve_chi2_batch_dev(weighted.handle, d_c, 64, 5, None, 0, d_o) == 0
    hip.mdns_dev_free(d_c)
    hip.mdns_dev_free(d_o)
    muse.close()
    weighted.close()


def test_a_fixed_scale_state_takes_curve_chunks_only(hip):
    ndata, nlive, nx = 20, 8, 64
    d = weighted_data(ndata, nx, seed=11, masked=True)
    spectra = WeightedSpectra(d["x"], d["y"], d["v"])
    model = line_model(d["x"])
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(DeviceScorer(spectra), nlive, ndata, model)
    rng = np.random.RandomState(3)
    rows5 = np.ones((nlive, 5))
    refused(hip.mdns_joint_init_muse3(dev._h, _lib.ptr(rows5), None), "mdns_joint_init_muse3", "curve chunks only")
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    dev.init(xs0)
    host.init(xs0)
    dev.prepare()
    host.prepare()
    accepted, nscored, npairs = C.c_int(7), C.c_int(0), C.c_int(0)
    bits = np.zeros(1, dtype=np.uint64)
    assert hip.mdns_backend_draw_begin(dev._h, None, ndata) == 0
    refused(hip.mdns_backend_draw_chunk(dev._h, _lib.ptr(rows5), 4, None, C.addressof(accepted), _lib.ptr(bits), C.addressof(nscored)),
             "mdns_backend_draw_chunk", "curve chunks only")
    assert accepted.value == -1
    refused(hip.mdns_backend_draw_score(dev._h, _lib.ptr(rows5), 4, None), "mdns_backend_draw_score", "curve chunks only")
    bound = np.zeros(4)
    status, pb, pk = (np.zeros(64, dtype=np.int32) for _ in range(3))
    pL, pt = np.zeros(64), np.zeros(64)
    refused(hip.mdns_backend_draw_band_begin(dev._h, _lib.ptr(rows5), 4, _lib.ptr(bound)), "mdns_backend_draw_band", "curve chunks only")
    refused(hip.mdns_backend_draw_band(dev._h, _lib.ptr(rows5), 4, _lib.ptr(bound), _lib.ptr(status), C.addressof(npairs), _lib.ptr(pb),
                                        _lib.ptr(pk), _lib.ptr(pL), _lib.ptr(pt), 64), "mdns_backend_draw_band", "curve chunks only")
    # ... and the state goes on as if nothing had happened: curve chunks decide as the statement does
    for attempt in range(6):
        cube = rng.uniform(size=(9, 3))
        cube[:, 0] *= 0.05
        xs = gauss_prior(cube)
        sel = None if attempt % 2 == 0 else np.arange(attempt % 3, ndata, 3)
        ia, _, ba, na = dev.draw(xs, sel)
        ib, _, bb, _ = host.draw(xs[:na], sel)
        assert ia == ib and (ia < 0 or np.array_equal(ba, bb)), attempt
        ha, hn = dev.thresholds()
        hb, hm = host.thresholds()
        assert np.array_equal(hn, hm) and np.array_equal(ha, hb)
    dev.close()
    spectra.close()
