"""Host orchestration (sampler, integrator, MLFriends constrainer, region, cache) against
golden traces recorded from the REFERENCE's own Python + C (oracle/make_trace.py).

The likelihood / geometry backends here are the CPU oracle (bit-identical to the reference C),
so everything must agree BIT-EXACTLY: per-iteration dead-point likelihoods and coordinates,
draw counts, final live-point id matrix, evidences, and the position of the global RNG stream.
"""
import os

import numpy as np
import pytest

from massivedatans_amd import gen, sample
from oracle_backend import OracleSpectra, patch_neighbors
from tracing import Recorder, check_bookkeeping, check_floats, load_trace
from chain_support import pow10_dd  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# horns100 = BASELINE.json configs[0] (100 spectra, 50 live points, 300 iterations: the run of
# SURVEY 3.3 with 44 272 likelihood calls); its fixture carries no per-iteration arrays
CASES = ["nothing4", "horns3", "horns12", "horns6", "horns100",
         # the reference's default grouping (USE_GRAPH=1) run through an igraph stand-in that
         # implements igraph's documented numbering only (oracle/make_trace.py)
         "nothing4_graph", "horns12_graph", "horns100_graph"]


def run_case(g, oracle, batched, fused=False, native=False, core=False):
    from massivedatans_amd.multi_nested_integrator import multi_nested_integrator
    ndata, nlive = int(g["ndata"]), int(g["nlive"])
    name = "horns" if "horns" in g["_name"] else "nothing"
    data = (gen.horns if name == "horns" else gen.nothing)(ndata)
    problem = sample.GaussLineProblem(data["x"], data["y"], backend=OracleSpectra(oracle, data["x"], data["y"]))
    sampler = sample.build_sampler(problem, nlive_points=nlive, nsuperset_draws=int(g["nsuperset_draws"]),
                                   use_graph=bool(g.get("use_graph", 0)), seed=1, batched=batched, fused=fused,
                                   native=native, core=core)
    assert (sampler.native is not None) == native
    assert (type(sampler).__name__ == "NativeCoreSampler") == core
    rec = Recorder(sampler)
    results = multi_nested_integrator(tolerance=0.5, multi_sampler=rec, min_samples=0,
                                      max_samples=int(g["max_samples"]))
    return results, sampler, rec, np.random.uniform()


# "fused": the likelihood matrix, the shelves' likelihoods, thresholds, accept test and shelf fill
# sit in a joint state (jointstate.HostJointState here: the numpy statement of what the GPU
# does) and the constrainers hand over whole chunks of candidates
@pytest.mark.parametrize("case", CASES)
# "native": the same with every constrainer a constrainer.NativeConstrainer -- region, proposals
# (numpy's own Mersenne Twister stepped in C), prior transform and accept loop of a draw in ONE call
# of csrc/host_constrainer.cpp, the oracle behind its backend table
# "core": the whole integer side of an iteration -- passes, grouping, constrainer cache, draws, shelves --
# behind mdns_core_fill (csrc/host_sampler.cpp), the constrainers inside it
# "native-chain" / "core-chain": the same two with the first batch of every fresh region handed over in one
# piece -- chain_begin / chain_end of the backend table, here the numpy statement of the device path
# (constrainer.chain_statement behind MDNS_PYTHON_BACKEND_CHAIN=1, the C library's pow): the host half of
# the hand-over (csrc/host_constrainer.cpp, BOX phase and the chain_valid branch of the draw) with its
# cross-checks, which no other CPU test reaches
@pytest.mark.parametrize("mode", ["single", "fused", "native", "core", "native-chain", "core-chain"])
def test_trace_bit_exact(case, mode, oracle, monkeypatch):
    g = load_trace(case)
    batched = mode != "single"
    chain = mode.endswith("-chain")
    if chain:
        monkeypatch.setenv("MDNS_PYTHON_BACKEND_CHAIN", "1")
        mode = mode[:-len("-chain")]
    if mode in ("native", "core"):
        from massivedatans_amd import constrainer
        if not constrainer.available():
            pytest.skip("libmdns_host.so not built")
    if case == "horns6" and mode not in ("single", "native", "core"):
        pytest.skip("242k draws: run one candidate at a time, native and core")
    if case.startswith("horns100") and mode == "single":
        pytest.skip("44k draws: run fused and native")
    patch_neighbors(monkeypatch, oracle)
    with np.errstate(all="ignore"):
        results, sampler, rec, rng_probe = run_case(g, oracle, batched, fused=(mode in ("fused", "native", "core")),
                                                    native=(mode in ("native", "core")), core=(mode == "core"))
    check_bookkeeping(g, sampler, rec, results)        # integers: ids, draw counts, accepted points
    check_floats(g, rec, results, rtol=0)              # floats: the same bits
    # the global legacy RNG stream was consumed call for call
    assert rng_probe == float(g["rng_probe"])
    # our own counter: every (candidate, data set) pair the sampler asked for
    assert sampler.nevals >= sampler.ndraws
    if sampler.native is not None:
        st = sampler.native.stats()
        # chained first batches happen with the switch and only with it; their accepted candidates were scored
        # with the host's own parameters.  (The cases looked at -- nothing4, horns3, horns12 -- never build a
        # region outside a draw or meet a chunk limit of 0, "chain_counts" stays 0 there, so it is not
        # asserted here: the counts-only route runs in tests/test_muse.py, mode native-chain.)
        assert (st["chains"] > 0) == chain and st["param_mismatch"] == 0, st
        if not chain:
            assert st["chain_counts"] == 0, st


def test_chained_trace_with_the_device_powers(oracle, monkeypatch, pow10_dd):
    """The chained first batches scored with the parameters the DEVICE computes: 10**v by ``pow10_dd``
    (csrc/mdns_pow10.h) instead of the C library's pow.  An accepted candidate whose parameter is one ulp
    off the host's keeps a likelihood that differs in its last bits (the documented behaviour of the
    device path; the accepted POINT is the host's own arithmetic either way), so the floats are compared
    to 1e-12 and the bookkeeping, which decides what a run does, must still be the reference's."""
    from massivedatans_amd import constrainer
    if not constrainer.available():
        pytest.skip("libmdns_host.so not built")
    monkeypatch.setenv("MDNS_PYTHON_BACKEND_CHAIN", "1")
    monkeypatch.setattr(constrainer, "CHAIN_POW10", pow10_dd)
    patch_neighbors(monkeypatch, oracle)
    g = load_trace("horns100")
    with np.errstate(all="ignore"):
        results, sampler, rec, rng_probe = run_case(g, oracle, True, fused=True, native=True, core=False)
    st = sampler.native.stats()
    print("horns100, chained with pow10_dd: %d chains, %d accepted candidates with parameters not the host's"
          % (st["chains"], st["param_mismatch"]))
    assert st["chains"] > 0
    check_bookkeeping(g, sampler, rec, results)
    check_floats(g, rec, results, rtol=1e-12)
    assert rng_probe == float(g["rng_probe"])


@pytest.mark.parametrize("fault,message", [("nkept", "the device kept"), ("chunk", "was scored, the host's is"),
                                           ("begin", "chain_begin failed")])
def test_host_cross_checks_of_the_chain_fire(fault, message, oracle, monkeypatch):
    """The host does not take the backend's word for the first batch (csrc/host_constrainer.cpp): it counts
    the kept proposals itself and sizes the chunk itself.  A statement that reports one kept proposal too
    many, a chunk one candidate short, or a failure must end the draw with the matching message, and
    the next constrainer of the same context draws as usual."""
    import ctypes as C
    from massivedatans_amd import constrainer, jointstate
    if not constrainer.available():
        pytest.skip("libmdns_host.so not built")
    monkeypatch.setenv("MDNS_PYTHON_BACKEND_CHAIN", "1")
    patch_neighbors(monkeypatch, oracle)
    ndata, nlive = 3, 40
    data = gen.horns(ndata)
    rng = np.random.RandomState(4)
    np.random.seed(4)
    joint = jointstate.HostJointState(OracleSpectra(oracle, data["x"], data["y"]), nlive, ndata, sample.kernel_params)
    pile_u = np.ascontiguousarray(rng.uniform(size=(nlive, 3)))
    joint.init(sample.priortransform_batch(pile_u))
    joint.prepare()
    be = constrainer.python_backend(joint)
    seen = {}

    def bad_begin(user, region, rq):
        return 1

    def bad_end(user, region, counts, nkept, B, accepted, bits, params):
        rc = be.chain_end(user, region, counts, nkept, B, accepted, bits, params)
        seen.update(nkept=nkept[0], B=B[0])
        if fault == "nkept":
            nkept[0] += 1
        else:
            B[0] -= 1
            if accepted[0] >= B[0]:
                accepted[0] = -1
        return rc

    wrapped = constrainer._CHAIN_BEGIN(bad_begin) if fault == "begin" else constrainer._CHAIN_END(bad_end)
    # the same table with one entry wrapped (a copy: the statement's own table stays as it is)
    bad = constrainer.DrawBackend()
    C.memmove(C.addressof(bad), C.addressof(be), C.sizeof(be))
    if fault == "begin":
        bad.chain_begin = wrapped
    else:
        bad.chain_end = wrapped
    prior = constrainer.sample_py_prior()
    ctx_bad = constrainer.NativeContext(bad, prior, ndata)
    ctx = constrainer.NativeContext(be, prior, ndata)
    settings = dict(metriclearner='truncatedscaling', force_shrink=True, rebuild_every=1000, metric_rebuild_every=20)
    con = ctx_bad.fresh_constrainer(**settings)
    with np.errstate(all="ignore"):
        with pytest.raises(RuntimeError) as err:
            con.draw_native(pile_u, np.arange(nlive), None, ndata)
        assert message in str(err.value), str(err.value)
        if fault != "begin":
            assert seen["nkept"] >= seen["B"] > 1, ("the fault would not show", seen)
        con.close()
        con = ctx.fresh_constrainer(**settings)
        u, x, tries, bits = con.draw_native(pile_u, np.arange(nlive), None, ndata)
        assert tries >= 1 and ((u > 0) & (u < 1)).all()
        assert con.stats()["chains"] == 1
        con.close()


def test_graph_grouping_is_the_same_partition(oracle, monkeypatch):
    """``generate_subsets_graph`` (connected components; its ORDER is pinned by the ``*_graph`` traces
    above, up to igraph's contract) must also produce the same PARTITION of data sets and live points as the pinned
    ``generate_subsets_nograph`` walk, on real sampler states where the data sets have split."""
    from massivedatans_amd.multi_nested_integrator import multi_nested_integrator
    patch_neighbors(monkeypatch, oracle)
    data = gen.horns(12)
    problem = sample.GaussLineProblem(data["x"], data["y"], backend=OracleSpectra(oracle, data["x"], data["y"]))
    sampler = sample.build_sampler(problem, nlive_points=24, nsuperset_draws=10, use_graph=False, seed=1, batched=False)
    checked = 0
    with np.errstate(all="ignore"):
        for it in range(120):
            next(sampler)
            if sampler.superpoints or it % 10:
                continue
            rng = np.random.RandomState(it)
            for mask in (np.ones(sampler.ndata, bool), rng.uniform(size=sampler.ndata) < 0.6):
                if mask.sum() < 2:
                    continue
                allp = np.unique(sampler.live_pointsp[:, mask])
                a = {(frozenset(np.flatnonzero(m).tolist()), frozenset(int(p) for p in pts))
                     for m, pts in sampler.generate_subsets_nograph(mask, allp)}
                b = {(frozenset(np.flatnonzero(m).tolist()), frozenset(int(p) for p in pts))
                     for m, pts in sampler.generate_subsets_graph(mask, allp)}
                assert a == b
                checked += len(a) > 1
    assert checked > 0, "no split state was reached: the test would be vacuous"


@pytest.mark.parametrize("core", [False, True])
def test_cached_gaussian_deviate_goes_back_to_numpy(core, oracle, monkeypatch):
    """numpy's legacy Gaussian generator caches the second deviate of a pair; the native constrainers
    continue the stream with their own copy of that cache (csrc/host_constrainer.cpp).  After a run
    numpy's own state must hold it again, so that Python code drawing afterwards stays on the
    reference's stream."""
    import ctypes as C
    from massivedatans_amd import constrainer
    if not constrainer.available():
        pytest.skip("libmdns_host.so not built")
    patch_neighbors(monkeypatch, oracle)
    monkeypatch.setenv("MDNS_NATIVE_CORE", "1" if core else "0")
    data = gen.horns(3)
    with np.errstate(all="ignore"):
        results, sampler, problem, _ = sample.run(data["x"], data["y"], nlive_points=20, max_samples=60,
                                                  backend=OracleSpectra(oracle, data["x"], data["y"]), fused=True)
    assert sampler.native is not None and (type(sampler).__name__ == "NativeCoreSampler") == core
    has, val = C.c_int(0), C.c_double(0)
    constrainer.host_lib().mdns_host_rng_get_gauss(C.addressof(has), C.addressof(val))
    st = np.random.get_state(legacy=False)
    assert int(st["has_gauss"]) == has.value
    if has.value:
        assert float(st["gauss"]) == val.value
    # and a draw from numpy now continues the pair: the cached deviate comes first
    expected = val.value if has.value else None
    got = np.random.normal()
    if expected is not None:
        assert got == expected
