"""The library's grow-only scratch (csrc/mdns_internal.h: DeviceBuffer, PinnedBuffer) growing on purpose.

The other GPU tests run many shapes in one process in whatever order pytest picks, so a block grows there by
accident.  Here every case runs in a fresh child process -- a cold library: every block starts empty -- and walks
ONE state through sizes in a fixed order: small, large (the blocks grow under a state that has already used them),
small again (the grown blocks at a small size), larger still (they grow a second time).  The parent makes the
inputs and the expected outcome on the CPU -- ``jointstate.HostJointState`` over the CPU oracle, the oracle's
quadratic K6 -- and compares them with the JSON the child prints.  A stale ticket or stamp, a view of a freed block
or a block a size too small shows as a wrong accept decision, wrong fill bits or a wrong radius.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from massivedatans_amd import gen, jointstate, musefuse
from oracle_backend import OracleMuseSpectra, OracleSpectra

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, arrays, timeout=120):
    """``code`` in a fresh interpreter with ``arrays`` in an .npz (sys.argv[1]); returns the JSON of its last line."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "inputs.npz")
        np.savez(path, **arrays)
        out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + code, path],
                             capture_output=True, text=True, timeout=timeout, env=dict(os.environ, MDNS_POLL_TIMEOUT_S="15"))
    assert out.returncode == 0, out.stderr[-1500:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _bits(beats):
    return np.flatnonzero(beats).tolist()


def _walk(host, chunks):
    """The chunks through the host statement: [accepted index, rows it beats (positions in the selection), thresholds,
    shelf sizes] after every chunk."""
    host.prepare()
    out = []
    for params, rows, jitter in chunks:
        idx, _, beats, _ = host.draw_params(params, rows, jitter=jitter)
        thr, n = host.thresholds()
        out.append((idx, _bits(beats) if idx >= 0 else [], thr, n))
    return out


# ---------------------------------------------------------------- Gaussian-line joint state --------
# (B, M) of the chunks: the second needs 256 x 10 trail entries, more than the first allocation holds under the
# old policy (8 + 4 + 1024) and under the new one (a page of stamps: 1024); the fourth 1024 x 20, far more than
# 1.5 x 2560.  No chunk reaches the matrix-core filter (B >= 128 and M B >= 8 000 000): the lane route.
GAUSS_NDATA, GAUSS_NX, GAUSS_NLIVE = 1280, 16, 8
GAUSS_CHUNKS = [(8, 64), (256, 640), (8, 64), (1024, 1280), (32, 100)]
GAUSS_PLANT = [5, 200, None, 1000, 17]        # where the one acceptable candidate of a chunk sits (None: nowhere)


def _gauss_inputs():
    rng = np.random.RandomState(1280)
    data = gen.horns(GAUSS_NDATA)
    x, y = np.ascontiguousarray(data["x"][:GAUSS_NX]), np.ascontiguousarray(data["y"][:GAUSS_NX])
    # live points: lines about as high as the noise (0.01) inside the 16 channels -- which of them a spectrum likes
    # least depends on its noise, so the thresholds differ from spectrum to spectrum
    live = np.column_stack([rng.uniform(0.005, 0.03, GAUSS_NLIVE), rng.uniform(x[2], x[-3], GAUSS_NLIVE), rng.uniform(3, 10, GAUSS_NLIVE)])
    chunks = []
    for k, ((B, M), plant) in enumerate(zip(GAUSS_CHUNKS, GAUSS_PLANT)):
        # candidates nobody takes: broad lines fifty to a hundred high ...
        params = np.column_stack([rng.uniform(50, 100, B), rng.uniform(x[0], x[-1], B), rng.uniform(30, 60, B)])
        if plant is not None:
            # ... and one sharply better amplitude, about that of the highest live point: the data sets whose noise
            # suits it take it, the others do not
            params[plant] = [0.029 - 0.001 * k, live[k, 1] + 1.0, live[k, 2]]
        if M == GAUSS_NDATA:
            rows = None
        elif k == 4:
            rows = np.sort(rng.choice(GAUSS_NDATA, size=M, replace=False)).astype(np.int32)      # ragged, non-contiguous
        else:
            rows = np.arange(k * 7, k * 7 + M, dtype=np.int32)
        chunks.append((np.ascontiguousarray(params), rows, None))
    return x, y, live, chunks


@pytest.fixture(scope="module")
def gauss_case(oracle):
    x, y, live, chunks = _gauss_inputs()
    host = jointstate.HostJointState(OracleSpectra(oracle, x, y), GAUSS_NLIVE, GAUSS_NDATA, lambda p: p)
    host.init(live)
    return x, y, live, chunks, _walk(host, chunks)


GAUSS_CHILD = """
import json, numpy as np
from massivedatans_amd import jointstate
from massivedatans_amd.like import GaussLineSpectra
d = np.load(sys.argv[1])
sp = GaussLineSpectra(d['x'], d['y'], noise_level=0.01)
dev = jointstate.GaussJointState(sp, int(d['nlive']), lambda p: p, shelf_cap=4, fetch_rows=False, via_backend=bool(d['via_backend']))
dev.init(d['live'])
dev.prepare()
out = []
for k in range(int(d['nchunks'])):
    rows = d['rows%d' % k] if ('rows%d' % k) in d.files else None
    idx, _, beats, _ = dev.draw_params(d['params%d' % k], rows)
    thr, n = dev.thresholds()
    out.append([int(idx), np.flatnonzero(beats).tolist() if idx >= 0 else [], [float(t).hex() for t in thr], n.tolist()])
dev.close()
print(json.dumps(out))
"""


def _chunk_arrays(chunks):
    arrays = {"nchunks": len(chunks)}
    for k, (params, rows, jitter) in enumerate(chunks):
        arrays["params%d" % k] = params
        if rows is not None:
            arrays["rows%d" % k] = rows
        if jitter is not None:
            arrays["jitter%d" % k] = jitter
    return arrays


def _compare(got, want, chunks, rtol):
    assert len(got) == len(want)
    for k, ((idx, bits, thr, n), (widx, wbits, wthr, wn)) in enumerate(zip(got, want)):
        M = len(wthr) if chunks[k][1] is None else len(chunks[k][1])
        print("chunk %d: accepted %d (host %d), beats %d of %d" % (k, idx, widx, len(bits), M))
        assert idx == widx, k
        assert bits == wbits, k
        assert np.array_equal(n, wn), k
        thr = np.array([float.fromhex(t) for t in thr])
        assert np.allclose(thr, wthr, rtol=rtol, atol=0, equal_nan=True), k


@pytest.mark.parametrize("via_backend", [False, True])
def test_gauss_joint_state_blocks_grow_under_one_state(via_backend, gauss_case):
    """Trail, templates, compact selection and pinned staging of ONE Gaussian-line state grow twice (chunks of
    GAUSS_CHUNKS; the last on 100 ragged rows), through mdns_joint_draw_gauss and through the backend entry points:
    after every chunk the accepted index, the rows it beats and the shelf sizes exactly as ``HostJointState`` over the
    CPU oracle has them, the thresholds within the 1e-12 of tests/test_joint.py's oracle test."""
    x, y, live, chunks, want = gauss_case
    # (the test's own design, from the host statement alone: the planted candidate is THE accepted one, and it beats
    # some rows of its selection, not all)
    for k, (idx, bits, _, _) in enumerate(want):
        assert idx == (-1 if GAUSS_PLANT[k] is None else GAUSS_PLANT[k]), k
    assert sum(idx < 0 for idx, _, _, _ in want) <= 1 and want[1][0] >= 0 and want[3][0] >= 0
    assert 0 < len(want[1][1]) < 640 and 0 < len(want[3][1]) < 1280
    got = _child(GAUSS_CHILD, dict(_chunk_arrays(chunks), x=x, y=y, live=live, nlive=GAUSS_NLIVE, via_backend=via_backend))
    _compare(got, want, chunks, rtol=1e-12)


# ---------------------------------------------------------------- MUSE-style joint state -----------
MUSE_NDATA, MUSE_NX, MUSE_NLIVE = 1024, 32, 8
MUSE_CHUNKS = [(4, 32), (64, 512), (4, 32), (256, 1024)]      # d_dense, d_jitter and the template block grow twice


def _muse_inputs():
    rng = np.random.RandomState(1024)
    data = gen.muse_like(MUSE_NDATA, MUSE_NX)
    live = musefuse.priortransform_batch(rng.uniform(size=(MUSE_NLIVE, 5)))
    noise0 = rng.normal(0, 1e-5, size=(MUSE_NLIVE, MUSE_NDATA))
    chunks = []
    for k, (B, M) in enumerate(MUSE_CHUNKS):
        params = musefuse.priortransform_batch(rng.uniform(size=(B, 5)))
        rows = None if M == MUSE_NDATA else np.sort(rng.choice(MUSE_NDATA, size=M, replace=False)).astype(np.int32)
        chunks.append((np.ascontiguousarray(params), rows, rng.normal(0, 1e-5, size=(B, M))))
    return data, live, noise0, chunks


MUSE_CHILD = """
import json, numpy as np
from massivedatans_amd import jointstate
from massivedatans_amd.like import MuseSpectra
d = np.load(sys.argv[1])
sp = MuseSpectra(d['x'], d['y'], d['v'])
dev = jointstate.MuseJointState(sp, int(d['nlive']), shelf_cap=4)
dev.init(d['live'], jitter=d['noise0'])
dev.prepare()
out = []
for k in range(int(d['nchunks'])):
    rows = d['rows%d' % k] if ('rows%d' % k) in d.files else None
    idx, _, beats, _ = dev.draw_params(d['params%d' % k], rows, jitter=d['jitter%d' % k])
    thr, n = dev.thresholds()
    out.append([int(idx), np.flatnonzero(beats).tolist() if idx >= 0 else [], [float(t).hex() for t in thr], n.tolist()])
dev.close()
print(json.dumps(out))
"""


def test_muse_joint_state_blocks_grow_under_one_state(oracle):
    """The dense likelihood block, the jitter block and the templates of ONE MUSE-style state grow twice (chunks of
    MUSE_CHUNKS, a jitter block with every chunk): accepted index, beaten rows and shelf sizes exactly as
    ``HostJointState`` over the oracle's cmuselike has them (built as in tests/test_muse.py), thresholds within that
    test's 1e-10."""
    data, live, noise0, chunks = _muse_inputs()
    host = jointstate.HostJointState(musefuse._LinesScorer(OracleMuseSpectra(oracle, data["x"], data["y"], data["v"])), MUSE_NLIVE,
                                     MUSE_NDATA, musefuse.kernel_params, nparams=5)
    host.init(live, jitter=noise0)
    want = _walk(host, chunks)
    assert sum(idx < 0 for idx, _, _, _ in want) <= 1 and want[1][0] >= 0 and want[3][0] >= 0
    got = _child(MUSE_CHILD, dict(_chunk_arrays(chunks), x=data["x"], y=data["y"], v=data["v"], live=live, noise0=noise0,
                                  nlive=MUSE_NLIVE))
    _compare(got, want, chunks, rtol=1e-10)


# ---------------------------------------------------------------- context scratch ------------------
K6_POOLS = [100, 5000, 100, 9000]


K6_CHILD = """
import json, numpy as np
from massivedatans_amd.clustering import neighbors
d = np.load(sys.argv[1])
out = []
for k in range(int(d['npools'])):
    pts, masks = d['pts%d' % k], d['masks%d' % k]
    s, r = neighbors.MemberSet.bootstrapped(pts, masks, 10)            # pinned staging, workspace (K >= 640)
    s.close()
    chosen = np.ascontiguousarray(neighbors.unpack_bootstrap_masks(masks, 10))
    out.append([float(r).hex(), float(neighbors.bootstrapped_maxdistance_chosen(pts, chosen)).hex()])     # workspace, masks
print(json.dumps(out))
"""


def test_context_scratch_grows_between_radius_computations(oracle):
    """K6 on pools of K6_POOLS points in that order (3 dimensions, 10 rounds, packed choices): the context's
    workspace and pinned staging block grow twice under the region entry point (members and packed choice staged
    together); the same choice as the reference's f64 matrix through the one-shot entry point makes the packed-mask
    block grow twice as well.  Every radius bit-equal to the oracle's."""
    from massivedatans_amd.clustering import neighbors
    rng = np.random.RandomState(9000)
    arrays, want = {"npools": len(K6_POOLS)}, []
    for k, K in enumerate(K6_POOLS):
        pts = np.ascontiguousarray(rng.uniform(size=(K, 3)))
        np.random.seed(K + k)
        masks = neighbors.draw_bootstrap_masks(K, 10)
        chosen = np.ascontiguousarray(neighbors.unpack_bootstrap_masks(masks, 10))
        want.append(oracle.bootstrapped_maxdistance(pts, chosen))
        arrays.update({"pts%d" % k: pts, "masks%d" % k: masks})
    got = _child(K6_CHILD, arrays)
    assert len(got) == len(want)
    for k, (pair, w) in enumerate(zip(got, want)):
        assert [float.fromhex(r) for r in pair] == [w, w], (k, K6_POOLS[k])
