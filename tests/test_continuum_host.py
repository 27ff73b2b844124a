"""The per-spectrum polynomial continuum without a device: the float64 statement
(massivedatans_amd/continuum.py) against its longdouble evaluation and against numpy's least squares, its limits,
the generator, the redshift recovery the feature exists for, a short run on the CPU backend, and the error paths
of the Python layer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from massivedatans_amd import continuum, gen, musefuse, parallel, problem
from continuum_support import case, reference, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(300, 5), (511, 3), (1030, 4), (4096, 2)]                    # (nx, ndata)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("nx,ndata", SHAPES)
def test_float64_statement_equals_the_longdouble_one(nx, ndata, P):
    d = case(nx, ndata, P, 5)
    want = reference(d["x"], d["y"], d["v"], d["ypred"], P)
    got = continuum.loglike_statement(d["x"], d["y"], d["v"], d["ypred"], P)
    assert got[0].dtype == np.float64 and got[0].shape == (5, ndata) and got[2].shape == (5, ndata, P)
    err = rel_err(got[0], want[0])
    print("nx=%d P=%d: float64 against longdouble, L max rel err %.3g" % (nx, P, err))
    assert err < 1e-13


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_seven_channels_leave_room_for_the_device_bound(P):
    """nx = 7 with P = 4 leaves two degrees of freedom: yt is what remains of y after a cancellation of 1e3, and the
    float64 statement stands 1e-13 from the longdouble one instead of 1e-14 -- still two orders inside the 1e-11 the
    device kernel is held to at this shape (tests/test_continuum.py)."""
    d = case(7, 3, P, 5)
    want = reference(d["x"], d["y"], d["v"], d["ypred"], P)
    err = rel_err(continuum.loglike_statement(d["x"], d["y"], d["v"], d["ypred"], P)[0], want[0])
    print("nx=7 P=%d: float64 against longdouble, L max rel err %.3g" % (P, err))
    assert err < 1e-12


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("nx,ndata", SHAPES)
def test_statement_is_the_weighted_least_squares_minimum(nx, ndata, P):
    """numpy.linalg.lstsq on the sqrt(w)-scaled design [m, b_0..b_{P-1}]: where sum w mt^2 / sum w m^2 >= 1e-6 the
    1e-10 regulariser is negligible."""
    d = case(nx, ndata, P, 4)
    st = continuum.Statement(d["x"], d["y"], d["v"], P)
    L, s, coef, ratio = st.score(d["ypred"])
    assert np.all(ratio >= 1e-6), ratio.min()
    b = continuum.legendre_basis(d["x"], P)
    for i, m in enumerate(d["ypred"]):
        for k in range(ndata):
            sw = np.sqrt(1.0 / d["v"][:, k])
            A = np.column_stack([m] + list(b)) * sw[:, None]
            sol, res = np.linalg.lstsq(A, d["y"][:, k] * sw, rcond=None)[:2]
            r = d["y"][:, k] * sw - A @ sol
            want = -0.5 * np.dot(r, r)
            assert abs(L[i, k] - want) <= 1e-12 * abs(want), (i, k, L[i, k], want)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_a_template_of_ones_scores_as_the_continuum_alone(P):
    """m in the span of the basis: mt = 0 up to rounding, the 1e-10 keeps s from blowing up, L = -0.5 sum w yt^2."""
    d = case(300, 4, P, 1)
    st = continuum.Statement(d["x"], d["y"], d["v"], P)
    L = st.score(np.ones((1, 300)))[0][0]
    want = -0.5 * (st.w * st.yt * st.yt).sum(axis=-1)
    assert np.max(np.abs(L - want) / np.abs(want)) < 1e-13


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_the_flat_part_of_a_template_is_absorbed(P):
    """s (1 + lines) + c_0 and s lines + (c_0 + s) are the same family: both templates give the same L."""
    d = case(512, 5, P, 6)
    a = continuum.loglike_statement(d["x"], d["y"], d["v"], d["ypred"], P)[0]
    b = continuum.loglike_statement(d["x"], d["y"], d["v"], d["ypred"] - 1.0, P)[0]
    assert np.max(np.abs(a - b) / np.abs(a)) < 1e-11


def test_generator_keeps_its_bytes_without_a_continuum():
    a, b = gen.muse_like(5, 64), gen.muse_like(5, 64, continuum=0)
    assert sorted(a) == sorted(b) == ["scale", "v", "x", "y", "z"]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = gen.muse_like(5, 64, continuum=3)
    assert c["continuum_coef"].shape == (5, 3) and c["v"].tobytes() == a["v"].tobytes()
    added = (c["continuum_coef"] @ continuum.legendre_basis(c["x"], 3)).T
    assert np.allclose(c["y"] - a["y"], added, rtol=0, atol=1e-12)
    g = np.random.RandomState([5, 3]).normal(size=(5, 3))
    assert np.array_equal(c["continuum_coef"], a["scale"][:, None] * np.array([1.0, 1.0, 0.5]) * g)


@pytest.mark.parametrize("nx", [512, 1030])
def test_redshifts_are_found_under_a_continuum(nx):
    """A random quadratic per spaxel: with it profiled out the best of 41 redshifts lies within one grid step of the
    truth for all 12 spaxels; the plain scale-marginalised likelihood (the same code with the continuum fitted to
    nothing is not available: its numpy statement below) does not manage that."""
    cube = gen.muse_like(12, nx=nx, continuum=3)
    zs = np.linspace(0.0, 0.02, 41)
    templates = np.array([gen.muse_template(cube["x"], (0.0, z, 0.0, 1.0, 1.0)) for z in zs])
    L = continuum.ContinuumScorer(cube["x"], cube["y"], cube["v"], 3).loglike_batch(templates)
    step = zs[1] - zs[0]
    best = zs[np.argmax(L, axis=0)]
    assert np.all(np.abs(best - cube["z"]) <= step * (1 + 1e-9)), (best, cube["z"])
    # K2 as it stands (cmuselike.c:45-64), for the record of why: it misses some
    w, y = 1.0 / cube["v"].T, cube["y"].T
    s = np.einsum('kj,bj->bk', w * y, templates) / (1e-10 + np.einsum('kj,bj->bk', w, templates ** 2))
    plain = -0.5 * np.array([(w * (y - s[b][:, None] * templates[b]) ** 2).sum(axis=1) for b in range(len(zs))])
    found = int((np.abs(zs[np.argmax(plain, axis=0)] - cube["z"]) <= step * (1 + 1e-9)).sum())
    print("nx=%d: the plain likelihood finds %d of 12 redshifts, with the continuum profiled out 12" % (nx, found))


def test_a_short_run_on_the_cpu_backend(oracle, monkeypatch):
    from oracle_backend import patch_neighbors
    patch_neighbors(monkeypatch, oracle)                 # (the region kernels have no CPU form: the oracle's)
    d = gen.muse_like(8, nx=300, continuum=2)
    backend = continuum.ContinuumScorer(d["x"], d["y"], d["v"], 2)
    np.random.seed(1)
    with np.errstate(all="ignore"):
        results, sampler, prob, _ = musefuse.run(d["x"], d["y"], d["v"], nlive_points=30, max_samples=60, backend=backend,
                                                 native=False, continuum=2)
    assert prob.continuum == 2 and prob.backend is backend
    u, xs, L, w, mask = (np.array(t) for t in zip(*results["weights"]))
    assert len(L) >= 30 and L.shape[1] == 8 and mask.any() and np.all(np.isfinite(L[mask.astype(bool)]))
    assert np.all(np.isfinite(results["logZ"]))


def test_error_paths_of_the_python_layer(monkeypatch):
    d = gen.muse_like(4, nx=64)
    x, y, v = d["x"], d["y"], d["v"]
    # sharded backends fit no continuum
    with pytest.raises(ValueError, match="sharded"):
        parallel.ShardedMuse(x, y, v, lambda *a, **k: None, continuum=2)
    from massivedatans_amd import sample
    monkeypatch.setattr(sample, "distributed_setup", lambda: (0, 2))
    with pytest.raises(ValueError, match="sharded"):
        musefuse.distributed_backend(x, y, v, continuum=1)
    monkeypatch.undo()
    sharded = parallel.ShardedMuse.__new__(parallel.ShardedMuse)
    sharded.lines, sharded.ref, sharded.continuum = None, 1, 0
    with pytest.raises(ValueError, match="sharded"):
        musefuse.MuseProblem(x, y, v, backend=sharded, continuum=2)
    # continuum without variances
    with pytest.raises(ValueError, match="variances"):
        problem.CurveProblem(x, y, lambda xs: xs, lambda us: us, ndim=2, continuum=2)
    # backend and problem disagree
    backend = continuum.ContinuumScorer(x, y, v, 2)
    with pytest.raises(ValueError, match="continuum = 2"):
        musefuse.MuseProblem(x, y, v, backend=backend, continuum=3)
    with pytest.raises(ValueError, match="continuum"):
        musefuse.MuseProblem(x, y, v, backend=backend)
    with pytest.raises(ValueError, match="continuum"):
        problem.CurveProblem(x, y, lambda xs: xs, lambda us: us, ndim=2, v=v, continuum=1, backend=backend)
    assert musefuse.MuseProblem(x, y, v, backend=backend, continuum=2).continuum == 2
    # values that are not an integer in 0..4
    for bad in (5, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="0..4"):
            musefuse.MuseProblem(x, y, v, backend=backend, continuum=bad)
    # a spectrum without weight
    vv = v.copy()
    vv[:, 2] = np.inf
    with pytest.raises(ValueError, match="spectrum 2"):
        continuum.ContinuumScorer(x, y, vv, 2)


@pytest.mark.parametrize("value", ["5", "-1", "two", "1.5"])
def test_main_refuses_a_bad_muse_continuum(value, tmp_path):
    env = dict(os.environ, MUSE_CONTINUUM=value, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "massivedatans_amd.musefuse", str(tmp_path / "none.npz"), "4"], env=env, cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode != 0 and "MUSE_CONTINUUM" in out.stderr and "0..4" in out.stderr, out.stderr
