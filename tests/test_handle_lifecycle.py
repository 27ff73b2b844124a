"""Handles made, used and destroyed over and over (csrc/mdns_internal.h: handles own their blocks through DeviceBuffer
and PinnedBuffer; blocks made on first use come whole or not at all).

Every case runs in a fresh child process (this file started as a program: ``python tests/test_handle_lifecycle.py CASE
inputs.npz``) that goes four times through one cycle: create the handles of a kind, use them so that every block they
make on first use is made, destroy them.  The child prints what every cycle computed and the free device memory after
it (``torch.cuda.mem_get_info`` behind ``mdns_sync``).  The parent makes the inputs and the expected outcome on the CPU
-- ``jointstate.HostJointState`` over the oracle backends, ``constrainer.chain_statement``, the oracle's K6 and K3,
``continuum.py``, numpy and scipy -- and asserts: cycle 1 is what the CPU statement says, cycles 2 to 4 equal cycle 1
bit for bit, and the free memory after cycle 4 is the free memory after cycle 2 (the first cycle makes what lives as
long as the process: context scratch, result slabs, the region pool).  A block freed twice, a view of a freed block or
a lazy group half made shows as a wrong result or a fault of a later cycle; a block nobody frees shows as memory lost.
(That a failed allocation leaves nothing behind is tests/test_owners_host.py's: nothing here makes one fail.)
"""
import ctypes as C
import gc
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from massivedatans_amd import _lib, constrainer, continuum, gen, jointstate, musefuse  # noqa: E402

pytestmark = pytest.mark.gpu

CYCLES = 4
#: bytes by which the free device memory after cycle 4 may differ from that after cycle 2 (the parent commit: 0)
ALLOWED_DRIFT = 0
NDATA, NX, NLIVE, NBOOT = 130, 16, 8, 15


# ------------------------------------------------------------------------------------------ both sides --------
def chain_prior(x):
    """A line inside the window of ``x``: A = 0.02 u + 0.005, mu = (x[-1] - x[0]) u + x[0], sigma = 10**(0.5 u + 0.5)."""
    p = constrainer.Prior()
    p.ndim, p.nparams = 3, 3
    for k, (a, b, p10, kp10) in enumerate(((0.02, 0.005, 0, 0), (float(x[-1] - x[0]), float(x[0]), 0, 0), (0.5, 0.5, 0, 1))):
        p.a[k], p.b[k], p.pow10[k], p.kernel_pow10[k] = a, b, p10, kp10
    return p


def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=float).ravel()]


def _unhex(a, shape=None):
    out = np.array([float.fromhex(v) for v in a])
    return out if shape is None else out.reshape(shape)


def _bits(beats):
    return [] if beats is None else np.flatnonzero(beats).tolist()


def _state(st):
    thr, n = st.thresholds()
    return [_hex(thr), np.asarray(n).tolist()]


# ------------------------------------------------------------------------------------------ the children ------
def _rows(d, name):
    return d[name] if name in d.files else None


def child_k1(d):
    """Gaussian-line spectra and two joint states on them."""
    from massivedatans_amd.like import GaussLineSpectra
    from chain_support import make_request
    lib = _lib.require_device()
    out = []
    sp = GaussLineSpectra(d["x"], d["y"], noise_level=0.01)
    dev = jointstate.GaussJointState(sp, NLIVE, lambda p: p, shelf_cap=4, fetch_rows=False, via_backend=True)
    dev.init(d["live"])
    dev.prepare()
    # the chained first batch of a region (the chain group; its draw_begin makes the mapped candidate block)
    members, masks, u, rows = d["members"], d["masks"], d["u"], d["rows_chain"]
    K, ndim = members.shape
    M = len(rows)
    region = lib.mdns_backend_region_begin(dev._h, _lib.ptr(members), K, ndim, _lib.ptr(masks), NBOOT)
    assert region, _lib.last_error()
    dev._check(lib.mdns_backend_draw_begin(dev._h, _lib.ptr(rows), M), "draw_begin")
    rq = make_request(u, members.min(axis=0), members.max(axis=0), chain_prior(d["x"]), int(d["limit"]))
    dev._check(C.cast(lib.mdns_backend_chain_begin, constrainer._CHAIN_BEGIN)(dev._h, region, C.addressof(rq)), "chain_begin")
    counts = np.full(len(u), -7, dtype=np.int32)
    nkept, B, accepted, radius = C.c_int(-9), C.c_int(-9), C.c_int(-9), C.c_double(0)
    bits = np.zeros((M + 63) // 64 + 1, dtype=np.uint64)
    params = np.full((1024, 3), np.nan)
    dev._check(C.cast(lib.mdns_backend_chain_end, constrainer._CHAIN_END)(
        dev._h, region, counts.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nkept), C.byref(B), C.byref(accepted),
        bits.ctypes.data_as(C.POINTER(C.c_ulonglong)), params.ctypes.data_as(C.POINTER(C.c_double))), "chain_end")
    dev._check(lib.mdns_backend_region_radius(dev._h, region, C.byref(radius)), "region_radius")
    lib.mdns_backend_region_destroy(dev._h, region)
    beats = jointstate.unpack_fill_bits(bits, M)
    if accepted.value >= 0:
        dev.took(rows, beats)
    out.append(dict(counts=counts.tolist(), nkept=nkept.value, B=B.value, accepted=accepted.value, radius=radius.value.hex(),
                    beats=_bits(beats) if accepted.value >= 0 else [], params=_hex(params[:max(B.value, 0)]), state=_state(dev)))
    # backend draws without and with a selection
    for k in ("a", "b"):
        idx, _, beats, _ = dev.draw_params(d["params_" + k], _rows(d, "rows_" + k))
        out.append([int(idx), _bits(beats), _state(dev)])
    # a chunk in two halves (the votes)
    dev.score_backend(d["params_c"], d["rows_c"])
    votes = dev.votes()
    idx, _, beats = dev.commit_backend()
    out.append([votes.tolist(), int(idx), _bits(beats), _state(dev)])
    # accepted points pile up on shelves of four: the shelves are replaced by larger ones
    for k in range(int(d["nfill"])):
        idx, _, beats, _ = dev.draw_params(d["params_f%d" % k], None)
        out.append([int(idx), _bits(beats), _state(dev)])
    out.append(int(lib.mdns_joint_shelf_cap(dev._h)))
    dev.close()
    # a second state on the same spectra: the draw of mdns_joint_draw_gauss without the likelihood row (the commit's ticket)
    dev = jointstate.GaussJointState(sp, NLIVE, lambda p: p, shelf_cap=4, fetch_rows=False, via_backend=False)
    dev.init(d["live"])
    dev.prepare()
    idx, _, beats, _ = dev.draw_params(d["params_g"], None)
    out.append([int(idx), _bits(beats), _state(dev)])
    dev.close()
    sp.close()
    return out


def child_filter(d):
    """One chunk of 1024 candidates against 1280 spectra through the accept filter MDNS_K1_FILTER forces."""
    from massivedatans_amd.like import GaussLineSpectra
    sp = GaussLineSpectra(d["x"], d["y"], noise_level=0.01)
    dev = jointstate.GaussJointState(sp, NLIVE, lambda p: p, shelf_cap=4, fetch_rows=False, via_backend=False)
    dev.init(d["live"])
    dev.prepare()
    idx, _, beats, _ = dev.draw_params(d["params"], None)
    out = [int(idx), _bits(beats), _state(dev)]
    dev.close()
    sp.close()
    return out


def _band(st, params, bound):
    """mdns_backend_draw_band over all spectra -> (status per candidate, listed pairs)."""
    lib, B, cap = st._lib, len(params), 4096
    st._check(lib.mdns_backend_draw_begin(st._h, None, st.ndata), "draw_begin")
    status, npairs = np.zeros(B, dtype=np.int32), C.c_int(0)
    pb, pk, pL, pthr = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap)
    st._check(lib.mdns_backend_draw_band(st._h, _lib.ptr(params), B, _lib.ptr(bound), _lib.ptr(status), C.byref(npairs), _lib.ptr(pb),
                                         _lib.ptr(pk), _lib.ptr(pL), _lib.ptr(pthr), cap), "draw_band")
    return status, npairs.value


def _band_chunk(sp, d, live, params):
    """A MUSE-style joint state on ``sp``, one band chunk, the commit of its first clear candidate."""
    lib = sp._lib
    st = jointstate.MuseJointState(sp, NLIVE, shelf_cap=4)
    st.init(live)
    st.prepare()
    stats = (C.c_longlong * 4)()
    lib.mdns_muse_filter_stats(stats)
    before = list(stats)
    status, npairs = _band(st, params, np.zeros(len(params)))
    lib.mdns_muse_filter_stats(stats)
    out = dict(status=status.tolist(), npairs=npairs, filtered=int(stats[0] - before[0]))
    clear = np.flatnonzero(status == 1)
    if len(clear):
        bits = np.zeros((st.ndata + 63) // 64, dtype=np.uint64)
        st._check(lib.mdns_backend_draw_band_commit(st._h, int(clear[0]), _lib.ptr(np.zeros(st.ndata)), _lib.ptr(bits)), "draw_band_commit")
        out["beats"] = _bits(np.unpackbits(bits.view(np.uint8), bitorder="little")[:st.ndata])
    out["state"] = _state(st)
    st.close()
    return out


def child_k2(d):
    """Spectra with variances: a line list, continua set and taken back, joint states with band chunks, the matrix-core
    filter (MDNS_K2_FILTER=1 in the child's environment) once."""
    from massivedatans_amd.like import MuseSpectra
    lines = [tuple(r) for r in d["lines"]]
    sp = MuseSpectra(d["x"], d["y"], d["v"], lines=lines, ref=0)
    out = [_hex(sp.loglike_batch_lines(d["params"]))]
    for P in (2, 4, 0, 2):
        _lib.check(sp._lib.mdns_spectra_set_continuum(sp._h, P), "mdns_spectra_set_continuum")
        sp.continuum = P
        out.append(_hex(sp.continuum_fit(d["ypred"])[0] if P else sp.loglike_batch(d["ypred"])))
    out.append(_band_chunk(sp, d, d["live"], d["params"]))                 # continuum 2: the exact kernels alone
    _lib.check(sp._lib.mdns_spectra_set_continuum(sp._h, 0), "mdns_spectra_set_continuum")
    sp.continuum = 0
    out.append(_band_chunk(sp, d, d["live"], d["params"]))                 # no continuum: through the forced filter
    sp.close()
    return out


def child_groups(d):
    from massivedatans_amd.grouping import DeviceGroups
    dg = DeviceGroups(d["ids"])
    out = []
    for npoints, rows in ((int(d["npoints0"]), None), (int(d["npoints0"]), d["rows"])):
        out.append([[m.tolist(), p.tolist()] for m, p in dg.groups(rows, npoints)])
    dg.replace(d["rep_rows"], d["rep_slots"], d["rep_ids"])                # ids past 4096: both blocks double
    for rows in (None, d["rows"]):
        out.append([[m.tolist(), p.tolist()] for m, p in dg.groups(rows, int(d["npoints1"]))])
    out.append(dg.ids().tolist())
    dg.close()
    return out


def child_posterior(d):
    from massivedatans_amd.posterior import Posterior
    with Posterior(d["w"], d["L"], d["x"]) as post:
        s = post.summary(tuple(d["q"]))
        index, xd = post.resample(int(d["n"]), seed=int(d["seed"]), gather=True)
    return [{k: (np.asarray(v).tolist() if np.asarray(v).dtype.kind in "iu" else _hex(v)) for k, v in sorted(s.items())},
            np.asarray(index).tolist(), _hex(xd)]


def child_regions(d):
    """More regions alive at once than a result slab has slots; plain and bootstrapped by turns."""
    from massivedatans_amd.clustering import neighbors
    alive, out = [], []
    for k in range(int(d["nregions"])):
        pts, masks = d["pts%d" % k], d["masks%d" % k]
        if k % 2:
            ms, r = neighbors.MemberSet.bootstrapped(pts, masks, NBOOT)
        else:
            ms = neighbors.MemberSet(pts)
            r = ms.bootstrap_radius(np.ascontiguousarray(neighbors.unpack_bootstrap_masks(masks, NBOOT)))
        alive.append(ms)
        out.append([float(r).hex()])
    for k, ms in enumerate(alive):                                         # (every one still answers)
        out[k].append(np.asarray(ms.count(d["cands"])).astype(int).tolist())
    for ms in alive:
        ms.close()
    return out


def main(case, path):
    import torch
    d = np.load(path)
    lib = _lib.require_device()
    cycles, free = [], []
    for _ in range(CYCLES):
        cycles.append(globals()["child_" + case](d))
        gc.collect()
        _lib.check(lib.mdns_sync(), "mdns_sync")
        free.append(int(torch.cuda.mem_get_info()[0]))
    print(json.dumps(dict(cycles=cycles, free=free)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ------------------------------------------------------------------------------------------ the parent --------
from chain_support import pow10_dd  # noqa: E402,F401  (fixture)
from oracle_backend import OracleMuseSpectra, OracleSpectra  # noqa: E402


def _run(case, arrays, env=None, timeout=180):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "inputs.npz")
        np.savez(path, **arrays)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), case, path], capture_output=True, text=True, timeout=timeout,
                             env=dict(os.environ, MDNS_POLL_TIMEOUT_S="15", **(env or {})))
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    got = json.loads(out.stdout.strip().splitlines()[-1])
    cycles, free = got["cycles"], got["free"]
    assert len(cycles) == CYCLES and len(free) == CYCLES
    print("%s: free device memory after the cycles %s, cycle 4 - cycle 2 = %d bytes" % (case, free, free[3] - free[1]))
    for k in range(1, CYCLES):
        assert cycles[k] == cycles[0], "cycle %d differs from cycle 1" % (k + 1)
    assert abs(free[3] - free[1]) <= ALLOWED_DRIFT, free
    return cycles[0]


def _same_state(got, host, rtol):
    thr, n = host.thresholds()
    assert got[1] == n.tolist()
    assert np.allclose(_unhex(got[0]), thr, rtol=rtol, atol=0, equal_nan=True)


def _window():
    data = gen.horns(NDATA)
    return np.ascontiguousarray(data["x"][:NX]), np.ascontiguousarray(data["y"][:NX])


def _chunk(rng, x, live, B, plant, k):
    """Broad lines fifty to a hundred high, which no data set takes, and one all but absent line at ``plant``: the data
    sets without a line of their own in the window prefer it to every live point."""
    params = np.column_stack([rng.uniform(50, 100, B), rng.uniform(x[0], x[-1], B), rng.uniform(30, 60, B)])
    params[plant] = [1e-4 * (k + 1), live[k % len(live), 1] + 1.0, live[k % len(live), 2]]
    return np.ascontiguousarray(params)


def test_gauss_spectra_and_joint_states(oracle, pow10_dd):
    """Chained first batch, backend draws with and without a selection, a chunk in two halves, shelves of four that fill
    and are replaced, and a second state drawing without the likelihood row, on 130 spectra of 16 channels: accepted
    index, votes, beaten rows and shelf sizes exactly as ``HostJointState`` over the CPU oracle has them, thresholds
    within the 1e-12 of tests/test_joint.py; the chain's counts, kept proposals and parameters exactly as
    ``constrainer.chain_statement`` over the oracle's K6 and K3 says."""
    from massivedatans_amd.clustering import neighbors
    rng = np.random.RandomState(130)
    x, y = _window()
    live = np.column_stack([rng.uniform(0.005, 0.03, NLIVE), rng.uniform(x[2], x[-3], NLIVE), rng.uniform(3, 10, NLIVE)])
    members = np.ascontiguousarray(0.5 + 0.15 * rng.uniform(-1, 1, size=(40, 3)))
    np.random.seed(40)
    masks = neighbors.draw_bootstrap_masks(40, NBOOT)
    u = np.ascontiguousarray(rng.uniform(size=(100, 3)))
    ragged = lambda m: np.sort(rng.choice(NDATA, size=m, replace=False)).astype(np.int32)      # noqa: E731
    arrays = dict(x=x, y=y, live=live, members=members, masks=masks, u=u, limit=32, rows_chain=ragged(77),
                  params_a=_chunk(rng, x, live, 32, 5, 0), params_b=_chunk(rng, x, live, 17, 11, 1), rows_b=ragged(57),
                  params_c=_chunk(rng, x, live, 21, 3, 2), rows_c=ragged(57), nfill=5, params_g=_chunk(rng, x, live, 32, 7, 8))
    for k in range(5):
        arrays["params_f%d" % k] = _chunk(rng, x, live, 8, 2, 3 + k)
    # the CPU statement of the same walk, first
    host = jointstate.HostJointState(OracleSpectra(oracle, x, y), NLIVE, NDATA, lambda p: p)
    host.init(live)
    host.prepare()
    radius = oracle.bootstrapped_maxdistance(members, np.ascontiguousarray(neighbors.unpack_bootstrap_masks(masks, NBOOT)))
    props, counts, kept, params = constrainer.chain_statement(
        u, members.min(axis=0), members.max(axis=0), radius, lambda p: oracle.count_within_distance_of(members, radius, p), None, None,
        chain_prior(x), 32, pow10=pow10_dd)
    assert 0 < len(params) <= 32 and 0 < kept.sum() < len(u)               # (the design: some proposals are kept, not all)
    want = []

    def drawn(p, rows, plant=None):
        idx, _, beats, _ = host.draw_params(p, rows)
        assert plant is None or (idx == plant and 0 < beats.sum())
        want.append((int(idx), _bits(beats if idx >= 0 else None), host.thresholds()))
    drawn(params, arrays["rows_chain"])
    drawn(arrays["params_a"], None, 5)
    drawn(arrays["params_b"], arrays["rows_b"], 11)
    flags = host.score_params(arrays["params_c"], arrays["rows_c"])
    assert flags.any() and int(np.argmax(flags)) == 3
    want.append((3, _bits(host.commit(3)[1]), host.thresholds()))
    for k in range(5):
        drawn(arrays["params_f%d" % k], None, 2)
    assert host.thresholds()[1].max() > 4                                   # (the shelves of four are outgrown)
    host = jointstate.HostJointState(OracleSpectra(oracle, x, y), NLIVE, NDATA, lambda p: p)
    host.init(live)
    host.prepare()
    drawn(arrays["params_g"], None, 7)
    assert len(want[-1][1]) > 128                                           # (past the one-workgroup commit of a tile or two)

    def same(got_idx, got_bits, got_state, w):
        assert [got_idx, got_bits] == [w[0], w[1]] and got_state[1] == w[2][1].tolist()
        assert np.allclose(_unhex(got_state[0]), w[2][0], rtol=1e-12, atol=0, equal_nan=True)
    got = _run("k1", arrays)
    chain = got[0]
    assert chain["radius"] == float(radius).hex() and chain["counts"] == np.asarray(counts).astype(int).tolist()
    assert chain["nkept"] == int(kept.sum()) and chain["B"] == len(params)  # (the chunk rode along: a full chain)
    assert np.array_equal(_unhex(chain["params"], (-1, 3)).view(np.int64), params.view(np.int64))
    same(chain["accepted"], chain["beats"], chain["state"], want[0])
    same(got[1][0], got[1][1], got[1][2], want[1])
    same(got[2][0], got[2][1], got[2][2], want[2])
    assert got[3][0] == flags.tolist()
    same(got[3][1], got[3][2], got[3][3], want[3])
    for k in range(5):
        same(got[4 + k][0], got[4 + k][1], got[4 + k][2], want[4 + k])
    assert got[9] >= 8                                                      # (... and were replaced by larger ones)
    same(got[10][0], got[10][1], got[10][2], want[9])


@pytest.mark.parametrize("forced", ["1", "m"])
def test_accept_filter_blocks(forced, oracle):
    """The blocks the guarded accept filters make on first use (sums of squares of the templates; the matrix-core form's
    marks and tiled spectra), at the smallest shape the filters take: 1024 candidates against 1280 spectra, the form
    forced by MDNS_K1_FILTER.  Decision, beaten rows and shelf sizes as ``HostJointState`` over the CPU oracle."""
    rng = np.random.RandomState(1280)
    data = gen.horns(1280)
    x, y = np.ascontiguousarray(data["x"][:NX]), np.ascontiguousarray(data["y"][:NX])
    live = np.column_stack([rng.uniform(0.005, 0.03, NLIVE), rng.uniform(x[2], x[-3], NLIVE), rng.uniform(3, 10, NLIVE)])
    params = _chunk(rng, x, live, 1024, 1000, 0)
    host = jointstate.HostJointState(OracleSpectra(oracle, x, y), NLIVE, 1280, lambda p: p)
    host.init(live)
    host.prepare()
    idx, _, beats, _ = host.draw_params(params, None)
    assert idx == 1000 and 0 < beats.sum()
    got = _run("filter", dict(x=x, y=y, live=live, params=params), env={"MDNS_K1_FILTER": forced})
    assert got[:2] == [idx, _bits(beats)]
    _same_state(got[2], host, 1e-12)


K2_LINES = ((0.35, 1.0, 0.12), (0.7, 0.6, 0.15))


def _band_statement(host, live, params, got, rtol):
    host.init(live)
    host.prepare()
    flags = host.score_params(params, None)
    assert flags.any()
    assert got["npairs"] == 0 and got["status"] == flags.tolist()          # (no threshold within 1e-12 of a candidate)
    _, beats = host.commit(int(np.argmax(flags)))
    assert beats.any() and got["beats"] == _bits(beats)
    _same_state(got["state"], host, rtol)


def test_muse_spectra_continuum_and_band_chunks(oracle):
    """Spectra with variances and a list of two lines: likelihoods with the continuum set to 2, 4, 0 and 2 terms against
    the longdouble statement of continuum.py (tests/continuum_support.py: 1e-11) and the oracle's cmuselike (1e-10); a band
    chunk of a joint state with the continuum, and one without it through the forced matrix-core filter, against
    ``HostJointState`` over the same two CPU backends."""
    import continuum_support as cs
    rng = np.random.RandomState(16)
    d = cs.small_cube(NX, NDATA, 2, rng)
    x, y, v = d["x"], d["y"], d["v"]
    lines, ref = gen.check_lines(K2_LINES, 0)

    def draw(B):
        return np.column_stack([rng.uniform(-0.3, 0.5, B), rng.uniform(-0.05, 0.05, B), rng.uniform(-0.1, 0.1, B), rng.uniform(0.3, 1.5, B)])
    params, live = draw(9), draw(NLIVE)
    ypred = np.array([gen.muse_template(x, p, lines, ref) for p in params])
    plain = musefuse.TemplateScorer(OracleMuseSpectra(oracle, x, y, v), x, lines, ref)
    got = _run("k2", dict(x=x, y=y, v=v, lines=np.array(lines), params=params, live=live, ypred=ypred), env={"MDNS_K2_FILTER": "1"})
    every = np.ones(NDATA, dtype=bool)
    assert cs.rel_err(_unhex(got[0], (9, NDATA)), plain.loglike_batch(params, every)) <= 1e-10
    for k, P in enumerate((2, 4, 0, 2)):
        L = _unhex(got[1 + k], (9, NDATA))
        if P:
            assert cs.rel_err(L, cs.reference(x, y, v, ypred, P)[0]) <= cs.RTOL_L
        else:
            assert cs.rel_err(L, plain.loglike_batch(params, every)) <= 1e-10
    with_c = musefuse._LinesScorer(continuum.ContinuumScorer(x, y, v, 2, lines, ref))
    assert got[5]["filtered"] == 0 and got[6]["filtered"] == 1             # (the filter is not for a continuum; forced, it ran once)
    _band_statement(jointstate.HostJointState(with_c, NLIVE, NDATA, lambda p: p, nparams=4), live, params, got[5], 1e-10)
    _band_statement(jointstate.HostJointState(plain, NLIVE, NDATA, lambda p: p, nparams=4), live, params, got[6], 1e-10)


def test_groups_blocks_double(oracle):
    """An id matrix of 40 live points for 130 data sets grouped before and after ids past 4096 enter it (the per-id block
    and the mapped list of distinct ids double): the groups scipy's connected components and numpy.unique give."""
    from test_groups import clustered_ids, cpu_groups
    rng = np.random.RandomState(40)
    lp = clustered_ids(rng, 40, NDATA, 4, 700)
    rows = np.sort(rng.choice(NDATA, size=57, replace=False)).astype(np.int32)
    npoints0, npoints1 = int(lp.max()) + 1, 6000
    assert npoints0 <= 4096 < npoints1 and 40 * NDATA > 4096
    n = 100
    rep_rows = np.sort(rng.choice(NDATA, size=n, replace=False)).astype(np.int32)
    rep_slots = rng.randint(0, 40, size=n).astype(np.int32)
    rep_ids = rng.choice(np.arange(4096, npoints1), size=n, replace=True).astype(np.int32)
    lp2 = lp.copy()
    lp2[rep_slots, rep_rows] = rep_ids
    got = _run("groups", dict(ids=lp.astype(np.int32), rows=rows, npoints0=npoints0, npoints1=npoints1, rep_rows=rep_rows,
                              rep_slots=rep_slots, rep_ids=rep_ids))
    for k, (matrix, sel) in enumerate(((lp, np.arange(NDATA)), (lp, rows), (lp2, np.arange(NDATA)), (lp2, rows))):
        want = cpu_groups(matrix, sel)
        assert got[k] == [[m.tolist(), p.tolist()] for m, p in want], k
    assert got[4] == lp2.tolist()


def test_posterior_summary_and_resample():
    """Summary with quantiles and a resampling of 57 samples of 130 data sets against the numpy statement of
    tests/test_posterior.py (its tolerances)."""
    import test_posterior as tp
    w, L, x = tp.make(57, NDATA, 3, seed=57)
    n, seed = 50, 4321
    got = _run("posterior", dict(w=w, L=L, x=x, q=np.array(tp.Q), n=n, seed=seed))
    shapes = dict(nfinite=None, imaxL=None, log_norm=(NDATA,), ess=(NDATA,), mean=(NDATA, 3), std=(NDATA, 3), quant=(NDATA, 3, len(tp.Q)))
    summary = {k: (np.array(got[0][k]) if shapes[k] is None else _unhex(got[0][k], shapes[k])) for k in shapes}
    tp.check_summary(summary, tp.ref_summary(w, L, x, tp.Q), x, w, L, tp.Q)
    index, xd = np.array(got[1]), _unhex(got[2], (NDATA, n, 3))
    for d in range(NDATA):
        want, near = tp.ref_choice(w, L, d, seed, n)
        assert np.all(near[index[d] != want] < 1e-12), d
        assert np.array_equal(xd[d], x[index[d], d, :]) if want[0] >= 0 else np.all(np.isnan(xd[d]))


def test_regions_past_one_result_slab(oracle):
    """70 regions of 30 points alive at once -- a result slab has 64 slots --, plain and bootstrapped by turns: every
    radius bit-equal to the oracle's K6, every membership count the oracle's K3."""
    from massivedatans_amd.clustering import neighbors
    rng = np.random.RandomState(70)
    cands = np.ascontiguousarray(rng.uniform(size=(33, 3)))
    arrays, want = dict(nregions=70, cands=cands), []
    for k in range(70):
        pts = np.ascontiguousarray(rng.uniform(size=(30, 3)))
        np.random.seed(700 + k)
        masks = neighbors.draw_bootstrap_masks(30, NBOOT)
        r = oracle.bootstrapped_maxdistance(pts, np.ascontiguousarray(neighbors.unpack_bootstrap_masks(masks, NBOOT)))
        want.append([float(r).hex(), oracle.count_within_distance_of(pts, r, cands).astype(int).tolist()])
        arrays.update({"pts%d" % k: pts, "masks%d" % k: masks})
    assert _run("regions", arrays) == want
