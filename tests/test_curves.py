"""Caller-defined models on the GPU: the fixed-noise likelihood from model curves (csrc/mdns_curves.hip,
include/mdns.h mdns_curve_loglike_batch[_dev]) against its numpy statement, the bit contract of a (curve,
spectrum) pair, the joint state from curves (``jointstate.CurveJointState``: mdns_joint_init_curves,
mdns_backend_draw_curves[_dev]) against ``jointstate.HostJointState`` fed by the same kernel, and whole runs
through ``sample.run_model``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib, gen, jointstate, problem, sample
from massivedatans_amd.like import GaussLineSpectra, MuseSpectra
from chi2_support import _fma
from curves_support import (STAGE_EDGE_CASES, Chunks, StatementProblem, dev_batch, gauss_prior, line_model, muse_cut, selections,
                            selections_by_size)
from test_joint import _drive

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = 0.01
RTOL_L = 1e-12                      # tests/test_hip_parity.py's bar for a likelihood


def _statement(curves, y, noise=NOISE):
    """-0.5 * (((c[:, :, None] - y[None]) / noise)**2).sum(axis=1), a block of candidates at a time."""
    out = np.empty((len(curves), y.shape[1]))
    for b0 in range(0, len(curves), 32):
        c = curves[b0:b0 + 32]
        out[b0:b0 + 32] = -0.5 * (((c[:, :, None] - y[None]) / noise) ** 2).sum(axis=1)
    return out


class CurveScorer(object):
    """``loglike_batch(curves, mask)`` of a GaussLineSpectra handle: the curve kernel."""

    def __init__(self, spectra):
        self.spectra = spectra

    def loglike_batch(self, curves, data_mask=None):
        return self.spectra.loglike_batch_curves(curves, data_mask)


# every nx of {1, 7, 33, 64, 200, 201, 513}, every B of {1, 3, 17, 64, 257, 1024}, every ndata of {1, 7, 100, 1000}
@pytest.mark.parametrize("nx,B,ndata", [(1, 1, 1), (7, 3, 7), (33, 17, 100), (64, 64, 1000), (200, 257, 100), (201, 1024, 7),
                                        (513, 64, 100), (200, 3, 1000)])
def test_kernel_against_the_numpy_statement(nx, B, ndata, hip):
    rng = np.random.RandomState(nx * 1000 + B)
    x = np.linspace(400, 800, nx)
    y = rng.normal(0, 0.05, size=(nx, ndata))
    curves = rng.uniform(-0.1, 0.3, size=(B, nx))
    spectra = GaussLineSpectra(x, y, noise_level=NOISE)
    want = _statement(curves, y)
    for name, rows in selections_by_size(ndata, rng):
        ref = want if rows is None else want[:, rows]
        got = spectra.loglike_batch_curves(curves, rows)
        assert got.shape == ref.shape
        err = np.max(np.abs(got - ref) / np.abs(ref))
        print("nx=%d B=%d ndata=%d %s: max rel err %.3g" % (nx, B, ndata, name, err))
        assert err < RTOL_L, (name, err)
        # rows longer than the curves, device pointers: the same bits
        assert np.array_equal(dev_batch(hip, spectra, curves, 3, rows, "mdns_curve_loglike_batch_dev", (NOISE,)), got), name
    spectra.close()


def _chain(curve, y, noise=NOISE):
    """The kernel's chain for one pair in float64, operation by operation: d = c - y, acc = fma(d, d, acc) from +0 with
    the channels ascending, L = acc * scale with scale = -0.5 / (noise * noise)."""
    acc = 0.0
    for c, yy in zip(np.asarray(curve, dtype=float).tolist(), np.asarray(y, dtype=float).tolist()):
        d = c - yy
        acc = _fma(d, d, acc)
    return acc * (-0.5 / (noise * noise))


@pytest.mark.parametrize("nx,ndata,B", STAGE_EDGE_CASES)
def test_kernel_against_the_emulated_chain(nx, ndata, B):
    """mdns_curve_loglike_batch bit for bit with the chain of the file header, at the first, the last and the middle pair
    of the whole batch and of a ragged selection, over nx across the 32-channel stage edges, ndata across the tile's 64
    and 128 spectra and B across a wave's 8 and the tile's 32 candidates."""
    rng = np.random.RandomState(nx * 1000 + B)
    y = rng.normal(0, 0.05, size=(nx, ndata))
    curves = rng.uniform(-0.1, 0.3, size=(B, nx))
    spectra = GaussLineSpectra(np.linspace(400, 800, nx), y, noise_level=NOISE)
    for name, rows in selections(ndata, rng):
        if name not in ("all", "ragged"):
            continue
        got = spectra.loglike_batch_curves(curves, rows)
        ks = np.arange(ndata) if rows is None else rows
        M = len(ks)
        assert got.shape == (B, M)
        for b, m in {(0, 0), (B - 1, M - 1), (B // 2, M // 2)}:
            assert got[b, m] == _chain(curves[b], y[:, ks[m]]), (name, b, m)
    spectra.close()


def test_a_pair_has_one_value():
    """The value of (curve b, spectrum k) is the same bits whatever B, M, the position of either in its batch
    and the entry point: a batch of 1024, the pair alone, a permuted batch over a selection, the live matrix."""
    rng = np.random.RandomState(11)
    nx, ndata, B = 200, 100, 1024
    d = gen.horns(ndata)
    curves = rng.uniform(0, 0.2, size=(B, nx))
    spectra = GaussLineSpectra(d["x"], d["y"], noise_level=NOISE)
    whole = spectra.loglike_batch_curves(curves)
    for b, k in [(0, 0), (1023, 99), (517, 64), (31, 63), (32, 65), (700, 7)]:
        alone = spectra.loglike_batch_curves(curves[b:b + 1], np.array([k]))
        assert alone.shape == (1, 1) and np.array_equal(alone[0, 0], whole[b, k]), (b, k)
    perm = rng.permutation(B)
    sel = np.sort(rng.choice(ndata, size=37, replace=False))
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm], sel), whole[perm][:, sel])
    assert np.array_equal(spectra.loglike_batch_curves(curves[perm[:5]], sel[3:4]), whole[perm[:5]][:, sel[3:4]])
    nlive = 70
    js = jointstate.CurveJointState(spectra, nlive, lambda xs: curves[xs[:, 0].astype(int)])
    js.init(np.arange(300, 300 + nlive, dtype=float)[:, None])
    assert np.array_equal(js.live_matrix(), whole[300:300 + nlive])
    js.close()
    spectra.close()


def test_against_k1():
    """Curves of a Gaussian line made in numpy score like the built-in line kernel (both of its shapes)."""
    d = gen.horns(100)
    x = d["x"]
    spectra = GaussLineSpectra(x, d["y"], noise_level=NOISE)
    rng = np.random.RandomState(6)
    for B in (3, 40):
        params = sample.kernel_params(gauss_prior(rng.uniform(size=(B, 3))))
        curves = params[:, 0, None] * np.exp(-0.5 * ((params[:, 1, None] - x[None]) / params[:, 2, None]) ** 2)
        a, b = spectra.loglike_batch_curves(curves), spectra.loglike_batch(params)
        err = np.max(np.abs(a - b) / np.abs(b))
        print("B=%d: curves against K1, max rel err %.3g" % (B, err))
        assert err < 1e-12
    spectra.close()


def _line_spectra(ndata, nx):
    data = gen.horns(ndata)
    x = np.linspace(400, 800, nx) if nx > 200 else data["x"][:nx]
    y = np.ascontiguousarray(np.vstack([data["y"], data["y"][:1]])[:nx]) if nx > 200 else np.ascontiguousarray(data["y"][:nx])
    return x, y


@pytest.mark.parametrize("ndata,nlive,nx", [(1, 5, 200), (7, 9, 33), (100, 50, 200), (1000, 40, 201), (90, 150, 48)])
def test_joint_state_equals_its_numpy_statement(ndata, nlive, nx):
    rng = np.random.RandomState(ndata * 7 + nlive)
    x, y = _line_spectra(ndata, nx)
    spectra = GaussLineSpectra(x, y, noise_level=NOISE)
    model = line_model(x)
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(CurveScorer(spectra), nlive, ndata, model)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    dev.init(xs0)
    host.init(xs0)
    assert dev.nparams == 3 and np.array_equal(dev.live_matrix(), host.live_matrix())
    assert _drive(dev, host, ndata, rng, iterations=12, exact=True) > 0
    dev.close()
    spectra.close()


class SameShapeScorer(object):
    """``loglike_batch(curves, mask)`` of a MuseSpectra handle for the numpy statement.  The last bits of a
    scale-marginalised likelihood depend on the kernel instantiation that scored it and on the candidate's place in
    its pair (csrc/mdns_like.hip, muse_rows_variant), and the statement scores a chunk in pieces of 1, 2, 4 ...
    candidates: so ``begin`` scores the whole chunk once, in the shape the device state scores it in, and the
    pieces that follow are handed their rows of that block."""

    def __init__(self, spectra):
        self.spectra, self._block = spectra, None

    def begin(self, curves, data_mask):
        self._block = (np.array(curves), np.array(data_mask), self.spectra.loglike_batch(curves, data_mask))
        self._pos = 0

    def loglike_batch(self, curves, data_mask=None):
        if self._block is not None:
            whole, mask, L = self._block
            piece = slice(self._pos, self._pos + len(curves))
            if np.array_equal(mask, data_mask) and np.array_equal(whole[piece], curves):
                self._pos += len(curves)
                return L[piece]
        self._block = None
        return self.spectra.loglike_batch(curves, data_mask)


@pytest.mark.parametrize("noisy", [False, True])
def test_scale_marginalised_joint_state_equals_its_numpy_statement(noisy):
    ndata, nlive, nx = 60, 12, 96
    rng = np.random.RandomState(60 + noisy)
    d = muse_cut(ndata, nx)
    x = d["x"]
    spectra = MuseSpectra(x, d["y"], d["v"])

    def model(xs):
        # rows (A, mu, log10 sig) of sample.priortransform_batch: a line somewhere in the window, on a continuum
        xs = np.atleast_2d(xs)
        out = np.empty((len(xs), nx))
        for b, (A, mu, ls) in enumerate(xs):
            out[b] = 1.0 + 2 * A * np.exp(-0.5 * ((x - (x[0] + (mu - 400) / 400 * (x[-1] - x[0]))) / (2.0 + 3 * ls)) ** 2)
        return out
    scorer = SameShapeScorer(spectra)
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(scorer, nlive, ndata, model)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    noise0 = rng.normal(0, 1e-5, size=(nlive, ndata)) if noisy else None
    dev.init(xs0, jitter=noise0)
    host.init(xs0, jitter=noise0)
    assert np.array_equal(dev.live_matrix(), host.live_matrix())
    assert _drive(Chunks(dev, lambda xs: xs, noisy), Chunks(host, model, noisy, scorer), ndata, rng, iterations=8, exact=True) > 0
    dev.close()
    spectra.close()


def test_parameter_chunks_and_curve_chunks_mix():
    """On one fixed-noise state chunks of the built-in line (mdns_backend_draw_chunk: the chunk kernels compute the
    templates themselves) alternate with curve chunks.  The statement scores numpy curves with the curve kernel
    throughout, so the two differ by the templates' last bits: 1e-12 on state and thresholds, and the same
    decisions as long as no likelihood of the statement lies within 1e-9 (relative) of its threshold -- which
    is asserted for every chunk."""
    ndata, nlive = 150, 20
    rng = np.random.RandomState(8)
    d = gen.horns(ndata)
    x = d["x"]
    spectra = GaussLineSpectra(x, d["y"], noise_level=NOISE)
    model = line_model(x)
    scorer = CurveScorer(spectra)
    dev = jointstate.CurveJointState(spectra, nlive, model, shelf_cap=4)
    host = jointstate.HostJointState(scorer, nlive, ndata, model)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    dev.init(xs0)
    host.init(xs0)
    kinds = [0, 0]
    for it in range(6):
        a, b = dev.prepare(), host.prepare()
        assert np.array_equal(a[1], b[1]) and np.allclose(a[0], b[0], rtol=1e-12, atol=0)
        waiting = np.zeros(ndata, dtype=int)
        for attempt in range(300):
            # (three points waiting per data set: thresholds move up within an iteration, shelves outgrow their capacity)
            if (waiting >= 3).all():
                break
            empty = np.flatnonzero(waiting < 3)
            rows = None if attempt < 2 else np.sort(rng.choice(empty, size=rng.randint(1, len(empty) + 1), replace=False))
            every = np.arange(ndata) if rows is None else rows
            cube = rng.uniform(size=(int(rng.choice([1, 5, 40])), 3))
            if attempt > 12:
                cube[:, 0] *= 0.05
            xs = gauss_prior(cube)
            ha, hn = dev.thresholds()
            hb, hm = host.thresholds()
            assert np.array_equal(hn, hm) and np.allclose(ha[every], hb[every], rtol=1e-12, atol=0)
            # the precondition: the statement's own decision is not a close call
            mask = np.zeros(ndata, dtype=bool)
            mask[every] = True
            L = scorer.loglike_batch(model(xs), mask)
            assert np.min(np.abs(L - hb[every]) / np.abs(hb[every])) > 1e-9
            kind = (it + attempt) % 2
            kinds[kind] += 1
            if kind == 0:
                ia, _, ba, na = dev.draw_gauss_params(sample.kernel_params(xs), rows)
            else:
                ia, _, ba, na = dev.draw(xs, rows)
            ib, _, bb, _ = host.draw(xs[:na], rows)
            assert ia == ib, (it, attempt, kind, ia, ib)
            if ia >= 0:
                assert np.array_equal(ba, bb)
                waiting[every[ba]] += 1
        assert (waiting >= 3).all()
        dev.advance()
        host.advance()
        assert np.allclose(dev.live_matrix(), host.live_matrix(), rtol=1e-12, atol=0)
    assert min(kinds) >= 9                                  # at least three chunks per iteration, alternating
    dev.close()
    spectra.close()


_TENSOR_SCRIPT = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch                                  # first: one HIP runtime per process
torch.cuda.set_device(0)
import numpy as np
from massivedatans_amd import gen, jointstate
from massivedatans_amd.like import GaussLineSpectra
from curves_support import gauss_prior, line_model
ndata, nlive, nx = 100, 30, 200
d = gen.horns(ndata)
spectra = GaussLineSpectra(d["x"], d["y"], noise_level=0.01)
as_numpy = line_model(d["x"])
calls = []
def as_tensor(xs):
    # rows of nx + 8 doubles on the device: read by pointer and row stride
    wide = torch.full((len(xs), nx + 8), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :nx] = torch.from_numpy(as_numpy(xs)).to("cuda")
    calls.append(wide.data_ptr())
    return wide[:, :nx]
a = jointstate.CurveJointState(spectra, nlive, as_numpy, shelf_cap=4)
b = jointstate.CurveJointState(spectra, nlive, as_tensor, shelf_cap=4)
rng = np.random.RandomState(9)
xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
a.init(xs0); b.init(xs0)
assert np.array_equal(a.live_matrix(), b.live_matrix())
accepted = 0
for it in range(5):
    pa, pb = a.prepare(), b.prepare()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    waiting = np.zeros(ndata, dtype=int)
    for attempt in range(300):
        if (waiting > 0).all():
            break
        empty = np.flatnonzero(waiting == 0)
        rows = None if attempt < 2 else np.sort(rng.choice(empty, size=rng.randint(1, len(empty) + 1), replace=False))
        every = np.arange(ndata) if rows is None else rows
        cube = rng.uniform(size=(int(rng.choice([1, 7, 64])), 3))
        if attempt > 6:
            cube[:, 0] *= 0.05
        xs = gauss_prior(cube)
        noise = rng.normal(0, 1e-7, size=(len(xs), len(every))) if attempt % 3 == 2 else None
        ia, _, ba, _ = a.draw_params(xs, rows, jitter=noise)
        ib, _, bb, _ = b.draw_params(xs, rows, jitter=noise)
        assert ia == ib, (it, attempt, ia, ib)
        if ia >= 0:
            accepted += 1
            assert np.array_equal(ba, bb)
            waiting[every[ba]] += 1
    assert (waiting > 0).all()
    ta, tb = a.thresholds(), b.thresholds()
    assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    a.advance(); b.advance()
    assert np.array_equal(a.live_matrix(), b.live_matrix())
assert accepted > 0 and len(calls) > 5
print("TENSOR OK", accepted, len(calls))
'''


def test_a_device_tensor_is_read_where_it_lies(tmp_path):
    """A model that returns a torch tensor on the device against the same curves returned as numpy: accepted
    indices, fill bits, thresholds and live matrix.  In a process of its own, torch imported first: the process
    must have one HIP runtime, and torch brings its own."""
    pytest.importorskip("torch")
    script = tmp_path / "curves_tensor.py"
    script.write_text(_TENSOR_SCRIPT)
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MDNS_DEVICE="0"))
    assert out.returncode == 0 and "TENSOR OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


@pytest.mark.parametrize("use_graph", [False, True])
def test_whole_run_equals_the_statement(use_graph):
    d = gen.horns(40)
    x, y = d["x"][96:160], np.ascontiguousarray(d["y"][96:160])
    model = line_model(x)
    runs = []
    for cls in (problem.CurveProblem, StatementProblem):
        p = cls(x, y, model, gauss_prior, 3, noise_level=NOISE)
        with np.errstate(all="ignore"):
            results, sampler, _, _ = sample.run_model(p, nlive_points=30, max_samples=60, use_graph=use_graph, seed=1)
        assert type(sampler.joint).__name__ == ("CurveJointState" if cls is problem.CurveProblem else "HostJointState")
        assert sampler.native is not None
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
    assert runs[0][2] > 0 and runs[0][2] == runs[1][2]
    for k in (0, 1, 3):
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_errors_leave_the_state_usable(hip):
    ndata, nlive = 20, 8
    d = gen.horns(ndata)
    x = d["x"]
    nx = len(x)
    spectra = GaussLineSpectra(x, d["y"], noise_level=NOISE)
    model = line_model(x)
    width = [nx]
    dev = jointstate.CurveJointState(spectra, nlive, lambda xs: np.ascontiguousarray(np.resize(model(xs), (len(xs), width[0]))), shelf_cap=4)
    host = jointstate.HostJointState(CurveScorer(spectra), nlive, ndata, model)
    rng = np.random.RandomState(2)
    xs0 = gauss_prior(rng.uniform(size=(nlive, 3)))
    dev.init(xs0)
    host.init(xs0)
    dev.prepare()
    host.prepare()
    accepted, nscored = C.c_int(7), C.c_int(0)
    bits = np.zeros(1, dtype=np.uint64)
    curves = np.zeros((_lib.JOINT_MAX_BATCH + 1, nx))
    out = (C.addressof(accepted), _lib.ptr(bits), C.addressof(nscored))
    # a curve chunk with no draw begun
    assert hip.mdns_backend_draw_curves(dev._h, _lib.ptr(curves), 4, None, *out) != 0
    assert "no draw begun" in _lib.last_error() and accepted.value == -1
    # more candidates than a chunk holds
    assert hip.mdns_backend_draw_begin(dev._h, None, ndata) == 0
    assert hip.mdns_backend_draw_curves(dev._h, _lib.ptr(curves), _lib.JOINT_MAX_BATCH + 1, None, *out) != 0
    assert "B=%d" % (_lib.JOINT_MAX_BATCH + 1) in _lib.last_error()
    d_c = hip.mdns_dev_alloc(curves.nbytes)
    assert hip.mdns_backend_draw_curves_dev(dev._h, d_c, nx, _lib.JOINT_MAX_BATCH + 1, None, *out) != 0
    assert "B=%d" % (_lib.JOINT_MAX_BATCH + 1) in _lib.last_error()
    assert hip.mdns_backend_draw_curves_dev(dev._h, d_c, nx - 1, 4, None, *out) != 0 and "channels" in _lib.last_error()
    hip.mdns_dev_free(d_c)
    # curves of the wrong width: caught before anything reaches the library
    xs = gauss_prior(rng.uniform(size=(9, 3)) * [0.05, 1, 1])
    width[0] = nx + 1
    with pytest.raises(ValueError):
        dev.draw(xs, None)
    width[0] = nx
    # ... and the state goes on as if nothing had happened
    ia, _, ba, na = dev.draw(xs, None)
    ib, _, bb, _ = host.draw(xs[:na], None)
    assert ia == ib and (ia < 0 or np.array_equal(ba, bb))
    ha, hn = dev.thresholds()
    hb, hm = host.thresholds()
    assert np.array_equal(hn, hm) and np.array_equal(ha, hb)
    dev.close()
    spectra.close()
