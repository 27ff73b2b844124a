"""The per-spectrum polynomial continuum on the GPU (csrc/mdns_continuum.hip, include/mdns.h Part 8): the scoring
kernel against the longdouble statement, the bit contract of a (template, spectrum) pair, the fit outputs, the C
ABI of mdns_spectra_set_continuum, the joint state and a whole run against their statements over the same
kernel, the matrix-core filter keeping out, and a caller-defined model."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib, continuum, gen, jointstate, musefuse, problem
from massivedatans_amd.like import GaussLineSpectra, MuseSpectra
from continuum_support import RTOL_L, Hidden, case, reference, rel_err, selection

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (P, nx, ndata, B, sparse selection?, kind): every P, every nx of {7, 300, 511, 512, 513, 1030, 2049, 4096} and 4100 (the
# generic form), every ndata of {1, 3, 70}, every B of {1, 2, 5, 33}; not nx = 7 at P = 4 with ndata = 1
CASES = [
    (1, 7, 1, 1, False, "muse"), (2, 7, 3, 2, False, "muse"), (3, 7, 70, 5, True, "muse"), (4, 7, 3, 33, False, "muse"),
    (1, 300, 70, 33, True, "muse"), (2, 300, 1, 1, False, "muse"), (3, 300, 3, 5, True, "muse"), (4, 300, 70, 2, False, "muse"),
    (2, 511, 3, 33, False, "muse"), (4, 511, 70, 5, True, "muse"),
    (1, 512, 70, 2, False, "muse"), (3, 512, 1, 33, False, "muse"),
    (2, 513, 70, 5, True, "muse"), (4, 513, 3, 1, False, "muse"),
    (1, 1030, 3, 5, True, "muse"), (3, 1030, 70, 33, False, "muse"), (4, 1030, 1, 2, False, "muse"),
    (1, 2049, 1, 1, False, "muse"), (2, 2049, 70, 33, True, "muse"), (4, 2049, 3, 5, False, "muse"),
    (1, 4096, 70, 5, False, "muse"), (2, 4096, 3, 2, True, "muse"), (3, 4096, 1, 5, False, "muse"), (4, 4096, 70, 33, True, "muse"),
    (1, 4100, 3, 33, False, "muse"), (2, 4100, 70, 5, True, "muse"), (3, 4100, 70, 2, False, "muse"), (4, 4100, 70, 33, True, "muse"),
    (2, 300, 70, 5, False, "nonuniform"), (3, 700, 3, 5, True, "nonuniform"),
    (3, 512, 70, 5, False, "masked"),
]


@pytest.mark.parametrize("P,nx,ndata,B,sparse,kind", CASES)
def test_kernel_against_the_statement(P, nx, ndata, B, sparse, kind):
    d = case(nx, ndata, P, B, kind=kind)
    rows = selection(ndata, sparse, np.random.RandomState(nx + ndata))
    spectra = MuseSpectra(d["x"], d["y"], d["v"], continuum=P)
    assert spectra.continuum == P and spectra._lib.mdns_spectra_continuum(spectra.handle) == P
    want = reference(d["x"], d["y"], d["v"], d["ypred"], P, rows)[0]
    got = spectra.loglike_batch(d["ypred"], rows)
    assert got.shape == want.shape == (B, ndata if rows is None else len(rows))
    err = rel_err(got, want)
    print("P=%d nx=%d ndata=%d B=%d %s %s: mdns_muse_loglike_batch max rel err %.3g" % (P, nx, ndata, B, "sparse" if sparse else "all", kind, err))
    assert err < RTOL_L
    if d["params"] is not None:
        # templates evaluated on the device from parameters: the statement on those templates
        templates = spectra.templates(d["params"])
        got2 = spectra.loglike_batch_lines(d["params"], rows)
        err2 = rel_err(got2, reference(d["x"], d["y"], d["v"], templates, P, rows)[0])
        print("    mdns_lines_loglike_batch max rel err %.3g" % err2)
        assert err2 < RTOL_L
        assert np.array_equal(got2, spectra.loglike_batch(templates, rows))          # one value per pair, whatever the entry point
    spectra.close()


def test_a_pair_has_one_value():
    """The bits of L for (template b, spectrum k) whatever B, M, the pair's place in its batch, the split of the
    candidates over the grid and the entry point: alone, inside B = 33, permuted, M = 1 against M = 70, and in the live
    matrix after mdns_joint_init_muse3."""
    for P, nx in ((3, 513), (2, 4100)):
        d = case(nx, 70, P, 33)
        spectra = MuseSpectra(d["x"], d["y"], d["v"], continuum=P)
        templates = spectra.templates(d["params"])
        whole = spectra.loglike_batch(templates)
        for b, k in [(0, 0), (32, 69), (17, 64), (1, 63), (16, 1)]:
            alone = spectra.loglike_batch(templates[b:b + 1], np.array([k]))
            assert alone.shape == (1, 1) and np.array_equal(alone[0, 0], whole[b, k]), (b, k)
            assert np.array_equal(spectra.loglike_batch(templates, np.array([k]))[:, 0], whole[:, k])       # M = 1 against M = 70
            assert np.array_equal(spectra.loglike_batch(templates[b:b + 1])[0], whole[b])                   # B = 1 against B = 33
        rng = np.random.RandomState(3)
        perm = rng.permutation(33)
        sel = np.sort(rng.choice(70, size=37, replace=False))
        assert np.array_equal(spectra.loglike_batch(templates[perm], sel), whole[perm][:, sel])
        assert np.array_equal(spectra.loglike_batch_lines(d["params"][perm[:5]], sel[3:4]), whole[perm[:5]][:, sel[3:4]])
        js = jointstate.MuseJointState(spectra, 33)
        js.init(d["params"])
        assert np.array_equal(js.live_matrix(), whole)
        js.close()
        spectra.close()


@pytest.mark.parametrize("P,nx,ndata,B", [(3, 511, 70, 5), (4, 4100, 3, 2), (1, 1030, 3, 5), (2, 7, 70, 2)])
def test_continuum_fit(P, nx, ndata, B):
    """L: the scoring call's bytes.  -0.5 sum w (y - s m - sum c_k b_k)^2 rebuilt in longdouble from the returned s and
    coef equals L to 1e-9 (the error of s enters at second order).  s and coef against the longdouble statement: within
    100 times the float64 statement's own largest deviation from it on the same inputs (the factor covers the other
    reduction order)."""
    d = case(nx, ndata, P, B)
    rows = selection(ndata, ndata > 3, np.random.RandomState(P))
    spectra = MuseSpectra(d["x"], d["y"], d["v"], continuum=P)
    L, s, coef = spectra.continuum_fit(d["ypred"], rows)
    assert np.array_equal(L, spectra.loglike_batch(d["ypred"], rows))
    ld = np.longdouble
    sel = np.arange(ndata) if rows is None else rows
    y, w = d["y"].T[sel].astype(ld), 1 / d["v"].T[sel].astype(ld)
    basis = continuum.legendre_basis(d["x"], P, ld)
    for b in range(B):
        r = y - s[b].astype(ld)[:, None] * d["ypred"][b].astype(ld) - coef[b].astype(ld) @ basis
        rebuilt = -0.5 * (w * r * r).sum(axis=-1)
        assert rel_err(L[b], rebuilt) < 1e-9, b
    want = reference(d["x"], d["y"], d["v"], d["ypred"], P, rows)
    f64 = continuum.loglike_statement(d["x"], d["y"], d["v"], d["ypred"], P, rows)
    for name, got, w_ld, w_64 in (("s", s, want[1], f64[1]), ("coef", coef, want[2], f64[2])):
        size = float(np.max(np.abs(w_ld)))
        own = float(np.max(np.abs(w_64 - w_ld))) / size
        dev = float(np.max(np.abs(got - w_ld))) / size
        print("P=%d nx=%d %s: float64 statement deviates %.3g from the longdouble one, the device %.3g (of the largest value)" % (P, nx, name, own, dev))
        assert dev <= 100 * own, (name, dev, own)
    spectra.close()


def test_set_continuum_at_the_c_abi(hip):
    d = gen.muse_like(5, 300, continuum=2)
    x, y, v = d["x"], d["y"], d["v"]
    templates = np.array([gen.muse_template(x, (0.0, z, 0.0, 1.0, 1.0)) for z in (0.001, 0.01, 0.015)])

    def refused(handle, P, word):
        rc = hip.mdns_spectra_set_continuum(handle, P)
        msg = _lib.last_error()
        assert rc != 0 and "mdns_spectra_set_continuum" in msg and word in msg, (rc, msg)

    sp = MuseSpectra(x, y, v)
    k2 = sp.loglike_batch(templates)
    refused(sp.handle, -1, "P=-1")
    refused(sp.handle, 5, "P=5")
    assert hip.mdns_spectra_continuum(sp.handle) == 0
    plain = GaussLineSpectra(x, y)
    refused(plain.handle, 2, "variances")
    plain.close()
    # P > 0 changes the bytes, P back to 0 restores K2's exactly
    assert hip.mdns_spectra_set_continuum(sp.handle, 2) == 0 and hip.mdns_spectra_continuum(sp.handle) == 2
    with_c = sp.loglike_batch(templates)
    assert not np.array_equal(with_c, k2) and np.all(with_c > k2)          # (a larger family fits at least as well)
    assert hip.mdns_spectra_set_continuum(sp.handle, 0) == 0 and hip.mdns_spectra_continuum(sp.handle) == 0
    assert np.array_equal(sp.loglike_batch(templates), k2)
    fresh = MuseSpectra(x, y, v)
    assert np.array_equal(fresh.loglike_batch(templates), k2)
    fresh.close()
    # the fit needs a continuum
    out = np.empty((3, 5))
    assert hip.mdns_muse_continuum_fit_batch(sp.handle, _lib.ptr(templates), 3, None, 5, _lib.ptr(out), None, None) != 0
    assert "continuum" in _lib.last_error()
    # once a joint state exists the model is fixed
    js = jointstate.MuseJointState(sp, 6)
    refused(sp.handle, 2, "joint state")
    js.close()
    assert hip.mdns_spectra_set_continuum(sp.handle, 1) == 0
    sp.close()
    # a spectrum without weight: the call fails, names it, and the handle goes on as before
    vv = v.copy()
    vv[:, 3] = np.inf
    bad = MuseSpectra(x, y, vv)
    before = bad.loglike_batch(templates)
    refused(bad.handle, 2, "spectrum 3")
    assert hip.mdns_spectra_continuum(bad.handle) == 0 and np.array_equal(bad.loglike_batch(templates), before)
    with pytest.raises(_lib.MdnsError, match="spectrum 3"):
        MuseSpectra(x, y, vv, continuum=2)
    bad.close()
    # fewer channels than terms
    tiny = MuseSpectra(x[:2], y[:2], v[:2])
    refused(tiny.handle, 3, "spectrum 0")
    tiny.close()


def _band_chunk(kb, dev, host, params, rows, rng, mode=-1):
    """One chunk through mdns_backend_draw_band (+ _commit) on the device state and through draw_params on the statement,
    with the noise a host would use: a row of |j| <= 4e-5 under the bound 4e-5 for a candidate the band settles, none
    for one it lists pairs of.  Returns the accepted index (or -1) and the data sets it filled."""
    B = len(params)
    M = dev.ndata if rows is None else len(rows)
    status, npairs, pb, pk, pL, pthr, _ = kb.band(dev, params, rows, np.full(B, 4e-5), mode)
    assert npairs <= 4096
    accepted, row = -1, np.zeros(M)
    for b in range(B):
        if status[b] == 1:
            accepted, row = b, np.clip(rng.normal(0, 1e-5, size=M), -4e-5, 4e-5)
            break
        if status[b] == 2 and np.any(pL[pb == b] > pthr[pb == b]):
            accepted = b
            break
    J = np.zeros((B, M))
    if accepted < 0:
        assert host.draw_params(params, rows, jitter=J)[0] == -1
        return -1, None
    J[accepted] = row
    bits = np.zeros((M + 63) // 64, dtype=np.uint64)
    dev._check(dev._lib.mdns_backend_draw_band_commit(dev._h, accepted, _lib.ptr(row), _lib.ptr(bits)), "mdns_backend_draw_band_commit")
    beats = np.unpackbits(bits.view(np.uint8), bitorder='little')[:M].astype(bool)
    dev.took(rows, beats)
    ib, _, bb, _ = host.draw_params(params, rows, jitter=J)
    assert ib == accepted and np.array_equal(bb, beats)
    return accepted, beats


@pytest.mark.parametrize("ndata,nlive", [(7, 20), (100, 40)])
def test_joint_state_equals_its_statement(ndata, nlive):
    """MuseJointState on spectra with a continuum against HostJointState over a scorer that calls the same kernel
    through the batch entry point: accepted indices, fill bits, live matrix and thresholds are equal, exactly -- through
    draw chunks with noise (mdns_backend_draw_chunk) and through the band form (mdns_backend_draw_band[_commit])."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k2_filter_bench as kb
    rng = np.random.RandomState(ndata)
    d = gen.muse_like(ndata, 300, continuum=2)
    spectra = MuseSpectra(d["x"], d["y"], d["v"], continuum=2)
    dev = jointstate.MuseJointState(spectra, nlive, shelf_cap=4)
    host = jointstate.HostJointState(musefuse._LinesScorer(Hidden(spectra)), nlive, ndata, musefuse.kernel_params, nparams=5)
    xs0 = musefuse.priortransform_batch(rng.uniform(size=(nlive, 5)))
    noise0 = rng.normal(0, 1e-5, size=(nlive, ndata))
    dev.init(xs0, jitter=noise0)
    host.init(xs0, jitter=noise0)
    assert np.array_equal(dev.live_matrix(), host.live_matrix())
    chunks = [0, 0]
    for it in range(4):
        a, b = dev.prepare(), host.prepare()
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
        waiting = np.zeros(ndata, dtype=int)
        for attempt in range(200):
            if (waiting > 0).all() and min(chunks) >= 2 * (it + 1):
                break
            empty = np.flatnonzero(waiting == 0)
            if attempt < 2 or len(empty) == 0:
                rows = None
            else:
                rows = np.sort(rng.choice(empty, size=rng.randint(1, len(empty) + 1), replace=False)).astype(np.int32)
            every = np.arange(ndata) if rows is None else rows
            route = attempt % 2
            chunks[route] += 1
            if route == 0:
                params = musefuse.priortransform_batch(rng.uniform(size=(int(rng.choice([1, 3, 9])), 5)))
                noise = rng.normal(0, 1e-5, size=(len(params), len(every)))
                ia, _, beats, _ = dev.draw_params(params, rows, jitter=noise)
                ib, _, bb, _ = host.draw_params(params, rows, jitter=noise)
                assert ia == ib, (it, attempt, ia, ib)
                if ia >= 0:
                    assert np.array_equal(beats, bb)
            else:
                params = musefuse.priortransform_batch(rng.uniform(size=(int(rng.choice([2, 5, 16])), 5)))
                ia, beats = _band_chunk(kb, dev, host, params, rows, rng)
            if ia >= 0:
                waiting[every[beats]] += 1
            ha, hn = dev.thresholds()
            hb, hm = host.thresholds()
            assert np.array_equal(hn, hm) and np.array_equal(ha, hb)
        assert (waiting > 0).all()
        dev.advance()
        host.advance()
        assert np.array_equal(dev.live_matrix(), host.live_matrix())
    assert min(chunks) >= 6, chunks
    spectra._lib.mdns_muse_filter_mode(-1)
    dev.close()
    spectra.close()


def test_the_matrix_core_filter_keeps_out(hip):
    """mdns_muse_filter_mode(1) sends EVERY band chunk of K2 through the filter; with a continuum the chunk of 16 x 600
    still takes the dense route, decides as the statement does, and the filter's counters do not move."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k2_filter_bench as kb
    ndata, nx, B, nlive = 600, 300, 16, 8
    rng = np.random.RandomState(16)
    d = gen.muse_like(ndata, nx, continuum=1)
    spectra = MuseSpectra(d["x"], d["y"], d["v"], continuum=1)
    dev = jointstate.MuseJointState(spectra, nlive)
    dev.init(musefuse.priortransform_batch(rng.uniform(size=(nlive, 5))))
    dev.prepare()
    thr = dev.thresholds()[0]
    params = musefuse.priortransform_batch(rng.uniform(size=(B, 5)))
    bound = np.full(B, 5e-5)
    s0 = kb.stats(hip)
    try:
        status, npairs, pb, pk, pL, pthr, _ = kb.band(dev, params, None, bound, 1)
        s1 = kb.stats(hip)
        assert s1 == s0, (s0, s1)
        # the statement's decision (float64, on the templates the device made); no pair of it is a close call
        L = continuum.ContinuumScorer(d["x"], d["y"], d["v"], 1).loglike_batch(spectra.templates(params))
        band = 1.01 * bound[:, None] + 1e-12 * (np.abs(L) + np.abs(thr)[None, :])
        for edge in (thr + band, thr - band):
            assert np.min(np.abs(L - edge) / np.abs(edge)) > 1e-9
        clear, inside = (L > thr + band).any(axis=1), ((L >= thr - band) & (L <= thr + band)).any(axis=1)
        assert np.array_equal(status, np.where(clear, 1, np.where(inside, 2, 0))) and (status == 1).any()
        assert npairs == int(((L >= thr - band) & (L <= thr + band)).sum())
        # the accept pass alone refuses
        d_t, d_thr, d_b, d_o = (hip.mdns_dev_alloc(n) for n in (B * nx * 8, ndata * 8, B * 8, 3 * B * 4 + 16))
        try:
            assert d_t and d_thr and d_b and d_o
            rc = hip.mdns_muse_filter_dev(spectra.handle, d_t, B, None, ndata, d_thr, d_b, d_o)
            assert rc != 0 and "continuum" in _lib.last_error()
        finally:
            for p in (d_t, d_thr, d_b, d_o):
                if p:
                    hip.mdns_dev_free(p)
    finally:
        hip.mdns_muse_filter_mode(-1)
    dev.close()
    spectra.close()


def test_a_whole_run_equals_the_statements_run():
    """musefuse.run on the default route (native core, state on the device) and with the spectra hidden behind a plain
    backend (HostJointState scoring chunk pieces through the batch entry point): the same samples, L, logZ and ndraws,
    exactly -- every pair has one value."""
    d = gen.muse_like(24, nx=300, continuum=2)
    out = []
    for hidden in (False, True):
        backend = Hidden(MuseSpectra(d["x"], d["y"], d["v"], continuum=2)) if hidden else None
        with np.errstate(all="ignore"):
            results, sampler, prob, _ = musefuse.run(d["x"], d["y"], d["v"], nlive_points=40, max_samples=120, continuum=2, backend=backend)
        joint = type(sampler.joint).__name__
        assert joint == ("HostJointState" if hidden else "MuseJointState"), joint
        assert hidden or (sampler.native is not None and prob.backend.continuum == 2)
        u, xs, L, w, mask = (np.array(t) for t in zip(*results["weights"]))
        out.append((u, xs, L, w, mask, np.array(results["logZ"]), np.array(results["logZerr"]), int(sampler.ndraws)))
        if hidden:
            assert backend.ncalls > 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert len(out[0][2]) >= 100 and np.all(np.isfinite(out[0][5]))


def test_a_caller_defined_model_with_a_continuum():
    """CurveProblem(..., v=v, continuum=2): the state made from the model's curves against ContinuumScorer on the same
    curves, to 1e-11 -- the initial live matrix, one draw chunk's decision and what it leaves in the live matrix."""
    ndata, nx, nlive = 40, 300, 12
    rng = np.random.RandomState(40)
    d = gen.muse_like(ndata, nx, continuum=2)
    x = d["x"]

    def model(xs):
        return np.array([gen.muse_template(x, p) for p in np.atleast_2d(xs)]).reshape(-1, nx)

    p = problem.CurveProblem(x, d["y"], model, musefuse.priortransform_batch, 5, v=d["v"], continuum=2)
    assert p.backend.continuum == 2
    scorer = continuum.ContinuumScorer(x, d["y"], d["v"], 2)
    js = p.joint_state(nlive)
    xs0 = musefuse.priortransform_batch(rng.uniform(size=(nlive, 5)))
    js.init(xs0)
    live = js.live_matrix()
    want = scorer.loglike_batch(model(xs0))
    assert rel_err(live, want) < RTOL_L
    Lmin, arg, _ = js.prepare()
    assert np.array_equal(arg, want.argmin(axis=0))
    xs = musefuse.priortransform_batch(rng.uniform(size=(8, 5)))
    Lc = scorer.loglike_batch(model(xs))
    assert np.min(np.abs(Lc - Lmin) / np.abs(Lmin)) > 1e-9               # (no close call in the statement)
    ok = (Lc > Lmin).any(axis=1)
    idx, _, beats, _ = js.draw(xs, None)
    assert ok.any() and idx == int(np.argmax(ok)) and np.array_equal(beats, Lc[idx] > Lmin)
    took = np.flatnonzero(beats).astype(np.int32)
    js.set_running(took)
    js.prepare()
    js.advance()
    after = js.live_matrix()
    assert after.shape == (nlive, len(took))
    assert rel_err(after[arg[took], np.arange(len(took))], Lc[idx][took]) < RTOL_L
    js.close()
    p.backend.close()
