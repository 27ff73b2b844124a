"""Test helpers of the guarded accept filters (test_filter_shapes.py, filter_cases.py) and of test_joint.py:
the filter modes and their children, the shape list, the input builder with its plain numpy reference in
``np.longdouble``, and ``_drive``, the sequence of iterations test_joint.py runs on a device state and its
numpy statement."""
import os
import subprocess
import sys

import numpy as np

from massivedatans_amd import sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: the project's own bar between a HIP likelihood and its high-precision statement (test_hip_parity.py)
RTOL_L = 1e-12
#: no reference likelihood of the ordinary and offset cases may lie this close (relative) to its threshold
CLEARANCE = 1e-9
NOISE = 0.01

#: filter mode -> what the child's environment adds; the library reads these once per process
MODES = {
    "1": {"MDNS_K1_FILTER": "1"},
    "mfma": {"MDNS_K1_FILTER": "mfma"},
    "mfma-lds": {"MDNS_K1_FILTER": "mfma", "MDNS_K1_FILTER_FORM": "lds"},
    "mfma-direct": {"MDNS_K1_FILTER": "mfma", "MDNS_K1_FILTER_FORM": "direct"},
    "mfma-ksplit": {"MDNS_K1_FILTER": "mfma", "MDNS_K1_GEMM_KSPLIT": "1"},
}
_SWITCHES = ("MDNS_K1_FILTER", "MDNS_K1_FILTER_FORM", "MDNS_K1_GEMM_KSPLIT", "MDNS_K1_GEMM_NC", "MDNS_K1_FILTER_BT",
             "MDNS_K1_BT", "MDNS_K1_PATH", "MDNS_CHUNK_PATH", "MDNS_CHUNK_GROUPS", "MDNS_FILTER_PROBE", "MDNS_TSQ_SHARES")
#: the mode of this process if it is a child of test_filter_shapes.py
MODE_VARIABLE = "MDNS_TEST_FILTER_MODE"
#: where the children of one session keep the references they share
CACHE_VARIABLE = "MDNS_TEST_FILTER_CACHE"

_FILTER_KERNEL = {"1": "k_gauss_cols_filter", "mfma": "k_gauss_gemm_filter", "mfma-lds": "k_gauss_mfma_filter",
                  "mfma-direct": "k_gauss_mfma_direct", "mfma-ksplit": "k_gauss_gemm_filter"}
#: the exact re-score behind the matrix-core forms holds a spectrum in 32 stages of 8 channels (k_exact_list<32>):
#: spectra with more padded channels stay on the chain kernel whatever MDNS_K1_FILTER says
EXACT_LIST_CHANNELS = 8 * 32


def expected_kernel(mode, nx):
    """Start of the name ``mdns_profile_kernel(0)`` must report after a draw chunk of ``nx`` channels under ``mode``."""
    if mode != "1" and (nx + 7) // 8 * 8 > EXACT_LIST_CHANNELS:
        return "k_gauss_cols_accept"
    return _FILTER_KERNEL[mode]


def child_environment(mode, cache=None):
    """Environment of the child that runs under filter ``mode``.  MDNS_K1_BT=8 lets the small shapes of these tests
    reach the filters (they engage from 8 candidates per wave on; the switch also moves the tile of the reference
    kernel, which does not change a likelihood).  MDNS_CHUNK_PATH=classic keeps the chunks of the backend entry
    points on the score the filters are part of: at these sizes they would otherwise all take the two-launch chunk,
    which has no filter."""
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(MODES[mode])
    env["MDNS_K1_BT"] = "8"
    env["MDNS_CHUNK_PATH"] = "classic"
    env[MODE_VARIABLE] = mode
    if cache is not None:
        env[CACHE_VARIABLE] = str(cache)
    return env


#: set once a child died by signal, abort or time limit: nothing more is started on the GPU after that
_child_died = []


def run_child(mode, path, cache=None, timeout=600, environment=child_environment):
    """One child pytest over ``path`` under filter ``mode``; once, never again.  Returns its output; raises
    AssertionError if it failed, died, or if an earlier child of this session died.  ``environment(mode, cache)``
    makes the child's environment (k2_filter_support.py passes its own)."""
    assert not _child_died, "not started: the child of mode %s died (%s)" % tuple(_child_died[0])
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", path]
    try:
        out = subprocess.run(cmd, env=environment(mode, cache), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _child_died.append((mode, "no end within %d s" % timeout))
        raise AssertionError("the child of mode %s did not end within %d s\n%s" % (mode, timeout, (e.stdout or b"")[-3000:]))
    tail = out.stdout[-6000:] + out.stderr[-2000:]
    if out.returncode < 0 or out.returncode >= 128:
        _child_died.append((mode, "exit status %d" % out.returncode))
        raise AssertionError("the child of mode %s died with exit status %d\n%s" % (mode, out.returncode, tail))
    assert out.returncode == 0 and " passed" in out.stdout and " failed" not in out.stdout and " skipped" not in out.stdout, tail
    return out.stdout


# ---------------------------------------------------------------------------------------
# Part A: shapes, inputs, reference
# ---------------------------------------------------------------------------------------
#: (ndata, selection, nx, B).  selection: None = every spectrum, "2/3" = two thirds of them, "1/10" = a tenth
#: (M * 8 < ndata: the sparse path), with the last spectrum and without the first.  What each shape is for:
SHAPES = [
    (1, None, 200, 17),        # one spectrum (M < 16: every tile ragged), B one past a candidate tile
    (17, None, 7, 1),          # one candidate, one channel group (nx <= 16), nxp = 8
    (63, None, 33, 15),        # M and B one short of a tile; 40 padded channels: the 40-channel chunk of the LDS form
    (65, "2/3", 64, 16),       # gather; four channel groups (even), two 32-channel chunks
    (257, None, 201, 33),      # M, nx and B one past a boundary; three candidate tiles (odd, two per wave: the clamp)
    (500, "1/10", 200, 48),    # sparse selection (M = 50), three candidate tiles, 13 channel groups (odd), five 40-channel chunks
    (1237, "2/3", 200, 130),   # nine candidate tiles: nc = 2 of the direct form with a ragged gy, three groups of the LDS form
    (1237, None, 8, 255),      # nxp = 8 (nk = 2), sixteen candidate tiles: nc = 4 of the direct form, B one short of a tile
    (2049, None, 1, 1024),     # nx = 1, the largest chunk; M one past a tile of 64
    (300, None, 256, 130),     # the last channel count k_exact_list<32> holds; 16 channel groups (even), eight 32-channel chunks
    (300, "2/3", 257, 130),    # the first one it does not; 17 groups (odd), seven 40-channel chunks (odd)
    (700, None, 300, 256),     # past it at a size the default rule takes with more spectra; 19 groups (odd), ten 32-channel chunks
    (130, "1/10", 520, 40),    # well past it, sparse (M = 13 < 16); 33 groups, thirteen 40-channel chunks
    # further branches the list above leaves out:
    (40, None, 16, 64),        # one channel group exactly (nxp = nxg = 16); M = 40: the second 32-spectrum tile of the LDS form ragged
    (200, None, 26 * 8, 20),   # k_exact_list<26> (nst = 26); 200 spectra: seven 32-spectrum tiles over the LDS form's eight XCD slots
    (100, "2/3", 120, 128),    # k_exact_list<16> (nst = 15); eight candidate tiles: the first nc = 2 of the direct form
]


def shape_id(shape):
    ndata, sel, nx, B = shape
    return "%dx%dx%d-%s" % (ndata, nx, B, {None: "all", "2/3": "two-thirds", "1/10": "tenth"}[sel])


def selection(ndata, sel, rng):
    """Ascending int32 row ids of the selection, or None for every spectrum."""
    if sel is None:
        return None
    if sel == "2/3":
        return np.sort(rng.choice(ndata, size=max(1, ndata * 2 // 3), replace=False)).astype(np.int32)
    m = max(2, ndata // 10)
    assert m * 8 < ndata
    rows = np.append(rng.choice(np.arange(1, ndata - 1), size=m - 1, replace=False), ndata - 1)
    return np.sort(rows).astype(np.int32)


def templates(x, params):
    """``A exp(-0.5 ((mu - x)/sig)^2)`` in float64, [B, nx]."""
    A, mu, sig = (params[:, k].reshape(-1, 1) for k in range(3))
    return A * np.exp(-0.5 * ((mu - x.reshape(1, -1)) / sig) ** 2)


def reference_loglike(x, y, params, noise=NOISE):
    """``L_ref[b, d] = -0.5/noise**2 * sum_j (m[b, j] - y[j, d])**2`` in ``np.longdouble``; y is [nx, ndata]."""
    m = templates(np.asarray(x, dtype=np.float64), np.asarray(params, dtype=np.float64)).astype(np.longdouble)
    yl = np.asarray(y).astype(np.longdouble)
    out = np.empty((len(m), yl.shape[1]), dtype=np.longdouble)
    scale = np.longdouble(-0.5) / (np.longdouble(noise) * np.longdouble(noise))
    for b in range(len(m)):
        out[b] = scale * ((m[b].reshape(-1, 1) - yl) ** 2).sum(axis=0)
    return out


def reference_resolution(x, y, params, noise=NOISE):
    """How far two correct float64 evaluations of ``L[b, d]`` may lie apart because their TEMPLATES differ: the
    reference's ``exp`` and the kernel's are each within one ulp of the true value, so within two of each other,
    and the product with A rounds once more in each: ``|dm| <= 3 * 2**-52 |m|`` per channel, which moves the sum by
    ``|scale| * 2 * sum_j |m_j - y_j| |dm_j|``.  Beside RTOL_L this is nothing (1e-14 |L| at 200 channels of noise)
    unless a template meets a spectrum of very few channels almost exactly (m - y cancels): float64 [B, ndata]."""
    m = templates(np.asarray(x, dtype=np.float64), np.asarray(params, dtype=np.float64))
    out = np.empty((len(m), y.shape[1]))
    for b in range(len(m)):
        mb = m[b].reshape(-1, 1)
        out[b] = (np.abs(mb - y) * np.abs(mb)).sum(axis=0)
    return out * (0.5 / noise ** 2 * 2 * 3 * 2.0 ** -52)


def make_inputs(shape, offset=0.0):
    """Grid, spectra [nx, ndata], candidates (A, mu, sig) [B, 3] and selection of a shape: noise plus one line for
    about four spectra in five, ``offset`` added to every channel; candidates spread over the grid."""
    ndata, sel, nx, B = shape
    rng = np.random.RandomState(1000 * nx + 7 * ndata + B)
    x = np.linspace(400, 800, nx) if nx > 200 else np.linspace(400, 800, 200)[:nx]
    lo, hi = x[0] - 2.0, x[-1] + 2.0
    y = rng.normal(0, NOISE, size=(nx, ndata))
    lined = rng.uniform(size=ndata) < 0.8
    A = np.where(lined, 0.02 / rng.power(3, size=ndata), 0.0)
    mu, sig = rng.uniform(lo, hi, size=ndata), 10 ** rng.uniform(0.3, 1.3, size=ndata)
    y += (A * np.exp(-0.5 * ((mu.reshape(1, -1) - x.reshape(-1, 1)) / sig) ** 2))
    y = np.ascontiguousarray(y + offset)
    params = np.column_stack([10 ** rng.uniform(-2, 0, size=B), rng.uniform(lo, hi, size=B), 10 ** rng.uniform(0, 2, size=B)])
    return x, y, np.ascontiguousarray(params), selection(ndata, sel, rng)


def reference(shape, offset=0.0):
    """``make_inputs`` and its ``L_ref`` [B, ndata], computed once per session (the children share it on disk)."""
    x, y, params, rows = make_inputs(shape, offset)
    cache = os.environ.get(CACHE_VARIABLE)
    path = os.path.join(cache, "%s-%g.npy" % (shape_id(shape), offset)) if cache else None
    if path and os.path.exists(path):
        L_ref = np.load(path)
    else:
        L_ref = reference_loglike(x, y, params)
        if path:
            np.save(path + ".%d.tmp.npy" % os.getpid(), L_ref)
            os.replace(path + ".%d.tmp.npy" % os.getpid(), path)
    return x, y, params, rows, L_ref


def unbeatable(L_ref):
    """Thresholds nobody beats: the best of every data set plus ``max(abs(L_ref)) * 1e-3`` of it, float64 [ndata]."""
    return (L_ref.max(axis=0) + np.abs(L_ref).max(axis=0) * np.longdouble(1e-3)).astype(np.float64)


def ordinary_thresholds(L_ref, rows):
    """Thresholds at a high percentile of every data set's reference likelihoods, between two neighbours of the
    sorted column: below the best candidate alone for most data sets, at the 97th percentile for one in sixteen --
    and at the next wide gap below where those two neighbours are closer than 1e-6 of their size (few channels: many
    candidates score alike) --, unbeatable ones for one data set in three.  So the accepted candidate is not simply the
    first, and it fills some shelves and not others.  Asserts, on the reference alone, that some candidate is
    accepted and that no pair of the selection lies within CLEARANCE of its threshold.  Returns float64 [ndata]."""
    B, ndata = L_ref.shape
    thr = unbeatable(L_ref)
    s = np.sort(L_ref, axis=0)
    for d in range(ndata):
        if d % 3 == 2 and ndata > 2:
            continue
        r = min(B - 1, int(0.97 * B)) if d % 16 == 0 else B - 1
        while r > 0 and not s[r, d] - s[r - 1, d] > 1e-6 * np.abs(s[r, d]):
            r -= 1
        below = s[r - 1, d] if r > 0 else s[0, d] - np.abs(s[0, d]) * np.longdouble(2e-3)
        thr[d] = np.float64((below + s[r, d]) / 2)
    sel = np.arange(ndata) if rows is None else rows
    t = thr[sel].astype(np.longdouble)
    L = L_ref[:, sel]
    assert (np.abs(L - t) > CLEARANCE * np.abs(L)).all(), "a reference likelihood within %g of its threshold" % CLEARANCE
    assert (L > t).any(), "no candidate is accepted"
    return thr


def decision(L, thr, rows):
    """(accepted index or -1, who it beats position by position) of likelihoods L [B, ndata] against thr [ndata]."""
    sel = np.arange(L.shape[1]) if rows is None else rows
    ok = L[:, sel] > thr[sel].astype(L.dtype)
    if not ok.any():
        return -1, None
    idx = int(np.argmax(ok.any(axis=1)))
    return idx, ok[idx]


# ---------------------------------------------------------------------------------------
# the whole joint state against its numpy statement
# ---------------------------------------------------------------------------------------
def _drive(dev, host, ndata, rng, iterations, exact):
    """The same sequence of iterations on both states: prepare, a few draw chunks on random
    selections until every running data set has something waiting, advance."""
    nlive = dev.nlive
    running = np.arange(ndata)
    ndraws = 0
    for it in range(iterations):
        if it == iterations // 2 and ndata > 8:
            running = np.sort(rng.choice(ndata, size=max(3, ndata * 2 // 3), replace=False))   # cut_down
            dev.set_running(running)
            host.set_running(running)
        a, b = dev.prepare(), host.prepare()
        assert np.array_equal(a[1], b[1])
        assert np.array_equal(a[0], b[0]) if exact else np.allclose(a[0], b[0], rtol=1e-12)
        assert (a[2] is None) == (b[2] is None)
        if a[2] is not None:
            w = min(a[2].shape[1], b[2].shape[1])
            assert np.array_equal(a[2][:, :w], b[2][:, :w]) and not a[2][:, w:].any() and not b[2][:, w:].any()
        waiting = np.zeros(ndata, dtype=int)
        waiting[running] = host.thresholds()[1][running]
        passes = 0
        while (waiting[running] == 0).any():
            passes += 1
            assert passes < 400, "the candidates never filled every shelf"
            if passes <= 2:
                rows = running                                      # superset draw
            else:
                empty = running[waiting[running] == 0]
                rows = np.sort(rng.choice(empty, size=rng.randint(1, len(empty) + 1), replace=False))
            B = int(rng.choice([1, 3, 17, 64, 200]))
            cube = rng.uniform(size=(B, 3))
            if passes > 6:
                cube[:, 0] *= 0.05                                  # faint lines beat more thresholds
            xs = sample.priortransform_batch(cube)
            ha, hn = dev.thresholds()
            hb, hm = host.thresholds()
            assert np.array_equal(hn[running], hm[running])
            assert np.array_equal(ha[running], hb[running]) if exact else np.allclose(ha[running], hb[running], rtol=1e-12)
            sel = None if len(rows) == ndata else rows
            xs = xs[:dev.chunk_size(len(xs), len(rows), hint=int(rng.randint(1, 80)))]
            ia, La, ba, na = dev.draw(xs, sel)
            ib, Lb, bb, nb_ = host.draw(xs[:na], sel)
            assert ia == ib, (it, passes, ia, ib)
            if ia >= 0:
                ndraws += 1
                assert np.array_equal(ba, bb)
                if La is not None:                                  # (None: the state keeps the row to itself)
                    assert np.array_equal(La, Lb) if exact else np.allclose(La, Lb, rtol=1e-12)
                waiting[rows[ba]] += 1
        dev.advance()
        host.advance()
        la, lb = dev.live_matrix(), host.live_matrix()
        assert np.array_equal(la, lb) if exact else np.allclose(la, lb, rtol=1e-12)
    return ndraws


class CountingState(object):
    """A device joint state that notes, after every draw, the chunk size and the kernel that scored it
    (``mdns_profile_kernel(0)``); everything else is the state's own."""

    def __init__(self, state, lib):
        self._state, self._lib = state, lib
        self.chunks = []                                       # (B, kernel name)

    def __getattr__(self, name):
        return getattr(self._state, name)

    def draw(self, xs, rows):
        out = self._state.draw(xs, rows)
        self.chunks.append((len(xs), (self._lib.mdns_profile_kernel(0) or b"").decode()))
        return out
