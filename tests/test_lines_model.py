"""The MUSE-style template with a caller-chosen emission-line list (gen.muse_template(x, params, lines, ref);
csrc/mdns_like.hip k_lines_model behind mdns_spectra_set_lines): the host statement, the problem definition that
derives from a list, the MUSE_LINES file -- without a GPU, over the CPU oracle's likelihood -- and, on the GPU, the
template kernel alone, the likelihoods, the joint state, the band / matrix-core filter paths and a whole run, each
against the host statement."""
import json
import os
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib, gen, musefuse
from oracle_backend import OracleMuseSpectra, patch_neighbors
from tracing import check_bookkeeping, check_floats
import lines_support as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# CPU tier
# ------------------------------------------------------------------------------------------------
def _muse_template_before(x, params):
    """gen.muse_template as it stood before it took a line list (three literal lines, five parameters)."""
    log_amp, z, log_ws, r1, r3 = params
    ratios = (r1, 1.0, r3)
    y = np.ones_like(x)
    for (mu, a, sg), r in zip(((4861.3, 0.35, 4.0), (5006.8, 1.0, 4.0), (6562.8, 0.8, 5.0)), ratios):
        y = y + (10 ** log_amp) * r * a * np.exp(-0.5 * ((x - mu * (1 + z)) / (sg * 10 ** log_ws)) ** 2)
    return y


def test_template_defaults_are_the_three_line_model_byte_for_byte():
    x = gen.muse_like(2, 777)["x"]
    rng = np.random.RandomState(3)
    for p in musefuse.priortransform_batch(rng.uniform(size=(20, 5))):
        want = _muse_template_before(x, p)
        assert gen.muse_template(x, p).tobytes() == want.tobytes()
        assert gen.muse_template(x, tuple(p)).tobytes() == want.tobytes()
        assert gen.muse_template(x, p, gen.MUSE_LINES, 1).tobytes() == want.tobytes()
    assert gen.MUSE_LINES == ((4861.3, 0.35, 4.0), (5006.8, 1.0, 4.0), (6562.8, 0.8, 5.0))


def test_muse_like_defaults_keep_their_bytes_and_take_a_list():
    """The default cube: the recipe of gen.muse_like written out with the three-line template as it stood; with a list the
    truth holds the list's lines."""
    n, nx = 4, 300
    x = np.linspace(4750, 9350, nx)
    rng = np.random.RandomState(n)
    z = rng.uniform(0.0, 0.02, size=n)
    scale = 10 ** rng.uniform(-1, 1, size=n)
    y, v = np.empty((nx, n)), np.empty((nx, n))
    for i in range(n):
        truth = scale[i] * _muse_template_before(x, (0.0, z[i], 0.0, 1.0, 1.0))
        v[:, i] = rng.uniform(0.5, 2.0, size=nx) * gen.NOISE_LEVEL ** 2
        y[:, i] = truth + rng.normal(0, 1, size=nx) * np.sqrt(v[:, i])
    d = gen.muse_like(n, nx)
    for k, want in (("x", x), ("y", y), ("v", v), ("z", z), ("scale", scale)):
        assert d[k].tobytes() == want.tobytes(), k
    lines, ref = ls.LISTS["two"]
    d2 = gen.muse_like(n, nx, lines=lines, ref=ref)
    assert np.array_equal(d2["v"], v) and np.array_equal(d2["z"], z)
    noise = y - scale * np.stack([_muse_template_before(x, (0.0, zi, 0.0, 1.0, 1.0)) for zi in z], axis=1)
    want = scale * np.stack([ls.restated_template(x, (0.0, zi, 0.0, 1.0), lines, ref) for zi in z], axis=1) + noise
    assert np.allclose(d2["y"], want, rtol=0, atol=1e-12 * scale.max() * 3)


@pytest.mark.parametrize("name", sorted(ls.LISTS))
def test_template_with_a_list_against_its_restatement(name):
    lines, ref = ls.LISTS[name]
    x = np.linspace(4750, 9350, 500)
    rng = np.random.RandomState(len(lines) + ref)
    for p in ls.physical(rng, 6, lines):
        assert len(p) == len(lines) + 2
        assert np.array_equal(gen.muse_template(x, p, lines, ref), ls.restated_template(x, p, lines, ref))


def test_template_parameter_order_and_ref():
    """A ratio moves exactly its own line: parameter 3 + k belongs to the k-th line that is not `ref`."""
    x = np.linspace(4750, 9350, 2000)
    lines = ((5000.0, 1.0, 10.0), (6000.0, 1.0, 10.0), (7000.0, 1.0, 10.0), (8000.0, 1.0, 10.0))
    for ref in (0, 2, 3):
        free = [g for g in range(4) if g != ref]
        base = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
        y0 = gen.muse_template(x, base, lines, ref)
        for k, g in enumerate(free):
            p = list(base)
            p[3 + k] = 2.0
            moved = np.abs(gen.muse_template(x, p, lines, ref) - y0)
            peak = [moved[np.argmin(np.abs(x - mu))] for mu, _, _ in lines]
            assert peak[g] > 0.9 and all(peak[h] < 1e-12 for h in range(4) if h != g), (ref, k, peak)
        # the reference line has no parameter: its height is the amplitude alone
        assert abs(y0[np.argmin(np.abs(x - lines[ref][0]))] - 2.0) < 0.01
    with pytest.raises(ValueError):
        gen.muse_template(x, (0.0, 0.0, 0.0, 1.0), lines, 0)              # 4 lines take 6 parameters
    with pytest.raises(ValueError):
        gen.muse_template(x, (0.0, 0.0, 0.0, 1.0, 1.0, 1.0))              # the default list takes 5


def test_problem_derives_names_count_and_prior_from_the_list():
    x = np.linspace(4750, 9350, 16)
    y = np.ones((16, 2))
    lines, ref = ls.LISTS["six-mid"]
    p = musefuse.MuseProblem(x, y, y, backend=object(), lines=lines, ref=ref,
                             prior=[None, (0.05, 0.01), None, None, (3.0, 0.0), None, None, None])
    assert p.nparams == 8 and p.paramnames == ['log_amp', 'z', 'log_width', 'ratio1', 'ratio2', 'ratio3', 'ratio5', 'ratio6']
    assert p.PRIOR == ((2.0, -1.0), (0.05, 0.01), (1.0, -0.5), (1.8, 0.2), (3.0, 0.0), (1.8, 0.2), (1.8, 0.2), (1.8, 0.2))
    u = np.random.RandomState(0).uniform(size=(5, 8))
    want = u * np.array([a for a, _ in p.PRIOR]) + np.array([b for _, b in p.PRIOR])
    assert np.allclose(p.priortransform_batch(u), want, rtol=1e-15)
    assert np.array_equal(p.priortransform(u[0]), p.priortransform_batch(u)[0])
    assert np.array_equal(p.model(want[0]), gen.muse_template(x, want[0], lines, ref))
    # without a list everything is the module's own
    q = musefuse.MuseProblem(x, y, y, backend=object())
    assert q.nparams == 5 and q.PRIOR is musefuse.PRIOR and q.paramnames == musefuse.paramnames
    assert np.array_equal(q.priortransform_batch(u[:, :5]), musefuse.priortransform_batch(u[:, :5]))
    with pytest.raises(ValueError):
        musefuse.MuseProblem(x, y, y, backend=object(), lines=lines, ref=ref, prior=[(1.0, 0.0)] * 5)
    with pytest.raises(ValueError):
        musefuse.MuseProblem(x, y, y, backend=object(), lines=lines, ref=6)


@pytest.fixture(scope="module")
def cpu_runs(oracle):
    """name -> the classic-orchestration run of the two-line problem over the CPU oracle's likelihood, as a trace (made once)."""
    made = {}

    def get(nx, max_samples, monkeypatch):
        key = (nx, max_samples)
        if key not in made:
            patch_neighbors(monkeypatch, oracle)
            lines, ref = ls.LISTS["two"]
            data = gen.muse_like(6, nx, lines=lines, ref=ref)
            out = ls.run(data, lines, ref, OracleMuseSpectra(oracle, data["x"], data["y"], data["v"]), fused=False, native=False,
                         nlive=20, max_samples=max_samples)
            assert out[1].native is None
            made[key] = (data, ls.as_trace(*out, nlive=20, ndata=6))
        return made[key]
    return get


def test_run_with_a_list_on_the_cpu_in_both_orchestrations(oracle, cpu_runs, monkeypatch):
    """A short complete run of a two-line problem (4 parameters) over the CPU oracle's cmuselike: one candidate per
    likelihood call through the Python constrainer, and whole chunks through the native core over
    HostJointState(TemplateScorer) -- the same integers, the same floats bit for bit, the random stream at the same place."""
    from massivedatans_amd import constrainer
    if not constrainer.available():
        pytest.skip("libmdns_host.so not built")
    data, g = cpu_runs(64, 150, monkeypatch)
    assert np.isfinite(g["logZ"]).all() and g["logZ"].shape == (6,) and g["nweights"] > 150
    patch_neighbors(monkeypatch, oracle)
    lines, ref = ls.LISTS["two"]
    results, sampler, rec, probe = ls.run(data, lines, ref, OracleMuseSpectra(oracle, data["x"], data["y"], data["v"]),
                                          fused=True, native=True, nlive=20, max_samples=150)
    assert sampler.native is not None and type(sampler.joint).__name__ == "HostJointState" and sampler.joint.nparams == 4
    assert isinstance(sampler.joint.scorer, musefuse.TemplateScorer)
    check_bookkeeping(g, sampler, rec, results)
    check_floats(g, rec, results, rtol=0)
    assert probe == g["rng_probe"]
    assert np.concatenate(rec.us).shape[1] == 4


def test_muse_lines_file_round_trip_and_rejections(tmp_path, monkeypatch):
    lines, ref = ls.LISTS["six-mid"]
    path = str(tmp_path / "lines.json")
    musefuse.write_lines(path, lines, ref)
    assert musefuse.read_lines(path) == (lines, ref, None)
    prior = musefuse.lines_prior(lines, [None, (0.05, 0.0)] + [None] * 6)
    musefuse.write_lines(path, lines, ref, prior)
    assert musefuse.read_lines(path) == (lines, ref, prior)
    with open(path, "w") as f:
        f.write('{"lines": [[6562.8, 1, 5], [6583.4, 0.3, 5.5]], "ref": 1}')
    assert musefuse.read_lines(path) == (((6562.8, 1.0, 5.0), (6583.4, 0.3, 5.5)), 1, None)
    seven = [[5000.0 + 100 * g, 1.0, 5.0] for g in range(7)]
    bad = {
        "no lines": {"lines": [], "ref": 0},
        "seven lines": {"lines": seven, "ref": 0},
        "ref past the end": {"lines": seven[:3], "ref": 3},
        "negative ref": {"lines": seven[:3], "ref": -1},
        "ref missing": {"lines": seven[:3]},
        "sigma zero": {"lines": [[5000.0, 1.0, 0.0]], "ref": 0},
        "sigma negative": {"lines": [[5000.0, 1.0, 5.0], [6000.0, 1.0, -2.0]], "ref": 0},
        "two numbers": {"lines": [[5000.0, 1.0]], "ref": 0},
        "not a number": {"lines": [[5000.0, "x", 1.0]], "ref": 0},
        "prior too short": {"lines": seven[:2], "ref": 0, "prior": [[1, 0]]},
        "unknown key": {"lines": seven[:2], "ref": 0, "lnes": 1},
        "a list": [1, 2, 3],
    }
    for why, spec in bad.items():
        with open(path, "w") as f:
            json.dump(spec, f)
        with pytest.raises(ValueError) as e:
            musefuse.read_lines(path)
        assert path in str(e.value), why
        # the command line: a message and exit, before any data is looked at
        monkeypatch.setenv("MUSE_LINES", path)
        with pytest.raises(SystemExit) as e:
            musefuse.main(["musefuse", str(tmp_path / "no-such-cube.npz"), "3"])
        assert isinstance(e.value.code, str) and "MUSE_LINES" in e.value.code and path in e.value.code, why
    with open(path, "w") as f:
        f.write("{not json")
    with pytest.raises(ValueError):
        musefuse.read_lines(path)
    with pytest.raises(ValueError):
        musefuse.read_lines(str(tmp_path / "absent.json"))


# ------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------
def _spectra(nx, lines, ref, ndata=2, seed=0):
    from massivedatans_amd.like import MuseSpectra
    rng = np.random.RandomState(seed)
    x = np.linspace(4750, 9350, nx)
    return x, MuseSpectra(x, rng.normal(1, 0.1, size=(nx, ndata)), rng.uniform(0.5, 2.0, size=(nx, ndata)) * 1e-4, lines=lines, ref=ref)


def _worst(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "two", "two-last", "three-mid", "six-first", "six-mid", "six-last"])
def test_template_kernel_against_the_host_statement(name):
    """mdns_lines_template_batch (k_lines_model<G> alone) against gen.muse_template: G in {1, 2, 3, 6}, ref first, middle and
    last; nx 333 (no multiple of 16), 1024 (one full block of 4 x 256), 1030 (a block and a ragged tail); B 1 and 17.
    rtol 1e-12 on the template value, atol 0: the continuum keeps every value >= 1, device exp / pow are within about
    2 ulp, the error of the exponent's argument is amplified by t^2 <~ 50 wherever the line term is above 1e-11 of the
    continuum: <~ 50 * 4 * 2.2e-16 * amp, about 1e-13 at amp <= 10.  Largest deviation seen on an MI355X: DESIGN section 4."""
    lines, ref = ls.LISTS[name]
    worst = 0.0
    for nx in (333, 1024, 1030):
        x, sp = _spectra(nx, lines, ref)
        assert sp.nparams == len(lines) + 2
        for B in (1, 17):
            params = ls.physical(np.random.RandomState(nx + B), B, lines)
            got = sp.templates(params)
            want = np.array([gen.muse_template(x, p, lines, ref) for p in params])
            assert got.shape == (B, nx) and (want >= 1).all() and want.max() > 1.01
            worst = max(worst, _worst(got, want))
            print("k_lines_model %s nx=%d B=%d: largest relative deviation %.3g" % (name, nx, B, _worst(got, want)))
            assert np.allclose(got, want, rtol=1e-12, atol=0), (name, nx, B, _worst(got, want))
        sp.close()
    print("k_lines_model %s: largest relative deviation %.3g" % (name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two", "six-mid"])
def test_likelihoods_of_a_list_against_k2_over_host_templates(name):
    """mdns_lines_loglike_batch against the exact K2 over templates made in numpy (MuseSpectra.loglike_batch), sparse mask."""
    lines, ref = ls.LISTS[name]
    ndata, nx, B = 70, 333, 9
    data = gen.muse_like(ndata, nx, lines=lines, ref=ref)
    from massivedatans_amd.like import MuseSpectra
    sp = MuseSpectra(data["x"], data["y"], data["v"], lines=lines, ref=ref)
    rng = np.random.RandomState(5)
    params = ls.physical(rng, B, lines)
    templates = np.array([gen.muse_template(data["x"], p, lines, ref) for p in params])
    for mask in (rng.uniform(size=ndata) < 0.3, None):
        got = sp.loglike_batch_lines(params, mask)
        want = sp.loglike_batch(templates, mask)
        assert got.shape == (B, ndata if mask is None else int(mask.sum())) and got.shape[1] > 5
        print("lines loglike %s: largest relative deviation %.3g" % (name, _worst(got, want)))
        assert np.allclose(got, want, rtol=1e-10, atol=0)
    with pytest.raises(ValueError):
        sp.loglike_batch_lines(np.zeros((2, 5 if len(lines) != 3 else 4)))
    sp.close()


@pytest.mark.gpu
def test_the_built_in_list_set_explicitly_and_another_list():
    """gen.MUSE_LINES set as a list: k_lines_model<3> gives the templates of k_muse3_model (to the tolerance of the template
    test); another list gives other templates -- a dispatch that ignored the table would not; G = 0 restores the built-in
    kernel bit for bit; bad lists and a list after a joint state are refused with a message."""
    from massivedatans_amd import jointstate
    nx, B = 1030, 17
    x, builtin = _spectra(nx, None, 1)
    _, same = _spectra(nx, gen.MUSE_LINES, 1)
    _, other = _spectra(nx, ((4861.3, 0.35, 4.0), (5100.0, 1.0, 4.0), (6562.8, 0.8, 5.0)), 1)
    assert builtin.nparams == same.nparams == other.nparams == 5 and builtin.lines is None
    params = musefuse.priortransform_batch(np.random.RandomState(8).uniform(size=(B, 5)))
    t0, t1, t2 = builtin.templates(params), same.templates(params), other.templates(params)
    print("k_lines_model<3> against k_muse3_model: largest relative deviation %.3g" % _worst(t1, t0))
    assert np.allclose(t1, t0, rtol=1e-12, atol=0)
    assert np.allclose(t0, [gen.muse_template(x, p) for p in params], rtol=1e-12, atol=0)
    assert _worst(t2, t0) > 1e-3
    assert np.allclose(t2, [gen.muse_template(x, p, other.lines, 1) for p in params], rtol=1e-12, atol=0)
    assert np.allclose(same.loglike_batch_lines(params), builtin.loglike_batch_lines(params), rtol=1e-10, atol=0)
    lib = other._lib
    # clearing: the built-in kernel again, the same bits as the handle that never had a list
    assert lib.mdns_spectra_set_lines(other.handle, None, 0, 0) == 0 and lib.mdns_spectra_nparams(other.handle) == 5
    out = np.empty((B, nx))
    _lib.check(lib.mdns_lines_template_batch(other.handle, _lib.ptr(params), B, _lib.ptr(out)), "mdns_lines_template_batch")
    assert np.array_equal(out, t0)
    table = np.array([[5000.0 + 100 * g, 1.0, 5.0] for g in range(7)])
    for G, ref, tab in ((7, 0, table), (3, 3, table), (3, -1, table), (-1, 0, table), (2, 0, np.array([[5000.0, 1.0, 0.0], [6000.0, 1.0, 1.0]])),
                        (2, 0, np.array([[5000.0, 1.0, 2.0], [6000.0, 1.0, -1.0]])), (1, 0, np.array([[np.nan, 1.0, 2.0]])),
                        (1, 0, np.array([[5000.0, np.inf, 2.0]]))):
        assert lib.mdns_spectra_set_lines(other.handle, _lib.ptr(np.ascontiguousarray(tab)), G, ref) != 0, (G, ref)
        assert b"mdns_spectra_set_lines" in lib.mdns_last_error() and lib.mdns_spectra_nparams(other.handle) == 5
    assert lib.mdns_spectra_set_lines(other.handle, _lib.ptr(table), 6, 5) == 0 and lib.mdns_spectra_nparams(other.handle) == 8
    js = jointstate.MuseJointState(other, 4)
    assert js.nparams == 8
    assert lib.mdns_spectra_set_lines(other.handle, _lib.ptr(table), 2, 0) != 0 and b"joint state" in lib.mdns_last_error()
    assert lib.mdns_spectra_set_lines(other.handle, None, 0, 0) != 0 and lib.mdns_spectra_nparams(other.handle) == 8
    js.close()
    assert lib.mdns_spectra_set_lines(other.handle, _lib.ptr(table), 2, 0) == 0 and lib.mdns_spectra_nparams(other.handle) == 4
    for sp in (builtin, same, other):
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two", "six-mid"])
def test_joint_state_with_a_list_against_its_numpy_statement(name, oracle):
    """The construction of test_muse_joint_state_against_its_numpy_statement with 4 and with 8 parameters: MuseJointState on
    the device against HostJointState over the numpy templates and the oracle's cmuselike -- live matrix, prepare, draw
    chunks with and without noise over full and sparse selections, fill bits, thresholds -- at that test's tolerances."""
    from massivedatans_amd import jointstate
    from massivedatans_amd.like import MuseSpectra
    lines, ref = ls.LISTS[name]
    nparams = len(lines) + 2
    rng = np.random.RandomState(12)
    ndata, nlive, nx = 70, 12, 333
    data = gen.muse_like(ndata, nx, lines=lines, ref=ref)
    spectra = MuseSpectra(data["x"], data["y"], data["v"], lines=lines, ref=ref)
    dev = jointstate.MuseJointState(spectra, nlive, shelf_cap=4)
    host = jointstate.HostJointState(musefuse.TemplateScorer(OracleMuseSpectra(oracle, data["x"], data["y"], data["v"]), data["x"], lines, ref),
                                     nlive, ndata, musefuse.kernel_params, nparams=nparams)
    assert dev.nparams == nparams
    xs0 = ls.physical(rng, nlive, lines)
    noise0 = rng.normal(0, 1e-5, size=(nlive, ndata))
    dev.init(xs0, jitter=noise0)
    host.init(xs0, jitter=noise0)
    assert np.allclose(dev.live_matrix(), host.live_matrix(), rtol=1e-10, atol=0)
    accepted = 0
    for it in range(4):
        a, b = dev.prepare(), host.prepare()
        assert np.array_equal(a[1], b[1]) and np.allclose(a[0], b[0], rtol=1e-10)
        waiting = np.zeros(ndata, dtype=int)
        for attempt in range(200):
            if (waiting > 0).all():
                break
            empty = np.flatnonzero(waiting == 0)
            rows = None if attempt < 2 else np.sort(rng.choice(empty, size=rng.randint(1, len(empty) + 1), replace=False)).astype(np.int32)
            M = ndata if rows is None else len(rows)
            B = int(rng.choice([1, 3, 9]))
            params = ls.physical(rng, B, lines)
            noise = rng.normal(0, 1e-5, size=(B, M)) if attempt % 2 == 0 else None
            ia, _, ba, _ = dev.draw_params(params, rows, jitter=noise)
            ib, _, bb, _ = host.draw_params(params, rows, jitter=noise)
            assert ia == ib, (it, attempt, ia, ib)
            if ia >= 0:
                accepted += 1
                assert np.array_equal(ba, bb)
                waiting[(np.arange(ndata) if rows is None else rows)[ba]] += 1
        assert (waiting > 0).all()
        ha, hn = dev.thresholds()
        hb, hm = host.thresholds()
        assert np.array_equal(hn, hm) and np.allclose(ha, hb, rtol=1e-10)
        dev.advance()
        host.advance()
        assert np.allclose(dev.live_matrix(), host.live_matrix(), rtol=1e-10, atol=0)
    assert accepted >= 4
    with pytest.raises(ValueError):
        dev.init(np.zeros((nlive, nparams + 1)))
    dev.close()
    spectra.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ndata,nx,B", [(600, 1024, 9), (1300, 333, 17)])
def test_band_and_filter_paths_with_four_parameters(ndata, nx, B):
    """test_k2_matrix_core_filter_decides_like_the_exact_kernels on its two small sparse shapes with a two-line list (4
    parameters per candidate; the block [B x 4 | B] of candidates and bounds): status, listed pairs and the commit are
    the same through the matrix-core filter and through the exact kernels, and both saw the candidates' own likelihoods
    (thresholds planted on them: a stride of 5 would score other candidates and settle nothing like this)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k2_filter_bench as kb
    lines, ref = ls.LISTS["two"]
    rng = np.random.RandomState(ndata + B)
    rows = np.sort(rng.choice(ndata, size=ndata * 2 // 3, replace=False)).astype(np.int32)
    results = {}
    lib = _lib.load()
    try:
        for mode in (1, 0):
            sp, st, params, L, thr = ls.planted_state(ndata, nx, 6, B, 5, [-1e-3, -1e-9, -1e-13, 0.0, 1e-13, 1e-9, 1e-3], lines, ref)
            assert params.shape == (B, 4) and st.nparams == 4
            s0 = kb.stats(lib)
            res = kb.band(st, params, rows, np.zeros(B), mode)
            s1 = kb.stats(lib)
            M = len(rows)
            bits = np.zeros((M + 63) // 64, dtype=np.uint64)
            first = int(np.flatnonzero(res[0] == 1)[0])
            st._check(lib.mdns_backend_draw_band_commit(st._h, first, _lib.ptr(np.zeros(M)), _lib.ptr(bits)), "draw_band_commit")
            higher, shelf_n = st.thresholds()
            results[mode] = (res[:6], bits.copy(), higher.copy(), shelf_n.copy(), [b - a for a, b in zip(s0, s1)], L, thr)
            st.close(); sp.close()
    finally:
        lib.mdns_muse_filter_mode(-1)
    exact, filt = results[0], results[1]
    assert np.array_equal(exact[0][0], filt[0][0])                     # status per candidate
    assert exact[0][1] == filt[0][1] and exact[0][1] > 0               # listed pairs: some thresholds are too close to call
    for a, b in zip(exact[0][2:], filt[0][2:]):
        assert np.array_equal(a, b)
    assert np.array_equal(exact[1], filt[1]) and np.array_equal(exact[2], filt[2]) and np.array_equal(exact[3], filt[3])
    assert exact[4][0] == 0 and filt[4][0] == 1 and filt[4][1] == 1 and filt[4][2] == 0
    assert (exact[0][0] == 1).any() and (exact[1] != 0).any()
    # the listed pairs carry the likelihoods of the stand-alone batch call for exactly those (candidate, data set) pairs
    _, npairs, pb, pk, pL, pthr = exact[0]
    assert np.allclose(pL, exact[5][pb, rows[pk]], rtol=1e-10, atol=0) and np.allclose(pthr, exact[6][rows[pk]], rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_run_with_a_list_on_the_gpu_against_the_cpu_statement(oracle, cpu_runs, monkeypatch):
    """musefuse.run with a two-line list on a cube that holds those lines, K2 joint state on the GPU under the native
    constrainer, against the same run over numpy templates and the CPU oracle's likelihood: the comparison of
    test_muse_on_the_gpu_against_the_reference_trace -- identical integers, the random stream at the same place, floats
    at rtol 1e-9."""
    lines, ref = ls.LISTS["two"]
    data = gen.muse_like(6, 256, lines=lines, ref=ref)
    results, sampler, rec, probe = ls.run(data, lines, ref, None, fused=True, native=True, nlive=20, max_samples=150)
    assert type(sampler.joint).__name__ == "MuseJointState" and sampler.native is not None and sampler.joint.nparams == 4
    _, g = cpu_runs(256, 150, monkeypatch)
    check_bookkeeping(g, sampler, rec, results)
    assert probe == g["rng_probe"]
    check_floats(g, rec, results, rtol=1e-9)
    assert np.isfinite(results["logZ"]).all()
    assert np.max(np.abs(results["logZ"] - g["logZ"]) / np.abs(g["logZ"])) < 1e-6
