"""Test helper of tests/test_lines_model.py: line lists, a numpy restatement of the template written
out independently of gen.muse_template, and runs of the MUSE-style analysis with a line list kept in
the form tests/tracing.py compares (check_bookkeeping / check_floats)."""
import numpy as np

from massivedatans_amd import gen, musefuse
from tracing import Recorder

#: (lines, ref) by name; wide lines, so that the coarse grids of the short runs resolve them
LISTS = {
    "one": (((6562.8, 1.0, 30.0),), 0),
    "two": (((6562.8, 1.0, 60.0), (8000.0, 0.5, 80.0)), 0),
    "two-last": (((5006.8, 0.7, 6.0), (6562.8, 1.0, 4.0)), 1),
    "three-mid": (((4861.3, 0.35, 4.0), (5006.8, 1.0, 4.0), (6562.8, 0.8, 5.0)), 1),
    "six-first": (((4861.3, 0.35, 4.0), (5006.8, 1.0, 4.0), (6548.1, 0.3, 5.0), (6562.8, 0.8, 5.0), (6583.4, 0.9, 5.0),
                   (6716.4, 0.25, 7.5)), 0),
    "six-mid": (((4861.3, 0.35, 40.0), (5006.8, 1.0, 40.0), (6548.1, 0.3, 50.0), (6562.8, 0.8, 50.0), (7200.0, 0.9, 50.0),
                 (8600.0, 0.25, 75.0)), 3),
    "six-last": (((4800.0, 0.35, 14.0), (5006.8, 1.0, 4.0), (6548.1, 0.3, 5.0), (7562.8, 0.8, 25.0), (8583.4, 0.9, 5.0),
                  (9300.0, 0.25, 7.5)), 5),
}


def restated_template(x, params, lines, ref):
    """1 + 10**log_amp * sum_g r_g a_g exp(-0.5 ((x - mu_g (1+z)) / (sigma_g 10**log_ws))**2), r_ref = 1, the
    ratios of the other lines in ascending order behind (log_amp, z, log_ws)."""
    log_amp, z, log_ws = params[0], params[1], params[2]
    free = list(params[3:])
    y = np.ones_like(x)
    for g, (mu, a, sg) in enumerate(lines):
        r = 1.0 if g == ref else free.pop(0)
        y = y + (10 ** log_amp) * r * a * np.exp(-0.5 * ((x - mu * (1 + z)) / (sg * 10 ** log_ws)) ** 2)
    assert not free
    return y


def physical(rng, B, lines):
    """B parameter rows drawn from the default prior of the list"""
    prior = musefuse.lines_prior(lines)
    return musefuse._transform_batch(rng.uniform(size=(B, len(prior))), prior)


def run(data, lines, ref, backend, fused, native, nlive, max_samples, nsuperset_draws=10, use_graph=False):
    """One analysis under the integrator; returns (results, sampler, recorder, the next uniform of the global stream)."""
    from massivedatans_amd import sample
    from massivedatans_amd.multi_nested_integrator import multi_nested_integrator
    problem = musefuse.MuseProblem(data["x"], data["y"], data["v"], backend=backend, jitter=True, lines=lines, ref=ref)
    sampler = sample.build_sampler(problem, nlive_points=nlive, nsuperset_draws=nsuperset_draws, use_graph=use_graph, seed=1,
                                   batched=False, fused=fused, native=native)
    rec = Recorder(sampler)
    with np.errstate(all="ignore"):
        results = multi_nested_integrator(tolerance=0.5, multi_sampler=rec, min_samples=0, max_samples=max_samples)
    if sampler.native is not None:
        sampler.native.sync_gauss_to_numpy()
    return results, sampler, rec, np.random.uniform()


def as_trace(results, sampler, rec, probe, nlive, ndata):
    """What a run left, under the keys of a golden trace (oracle/make_trace.py)."""
    return dict(iter_nrunning=np.array([len(L) for L in rec.Ls]), iter_ndraws=np.array(rec.ndraws_after), ndraws=sampler.ndraws,
                npoints=len(sampler.pointpile), nlive=nlive, ndata=ndata, final_live_pointsp=rec.term_p.copy(),
                nweights=len(results["weights"]), iter_u=np.concatenate(rec.us), iter_L=np.concatenate(rec.Ls),
                final_live_pointsL=rec.term_L.copy(), logZ=np.array(results["logZ"]), information=np.array(results["information"]),
                logZerr=np.array(results["logZerr"]), rng_probe=probe)


def planted_state(ndata, nx, nlive, B, seed, offsets, lines, ref):
    """tools/k2_filter_bench.py planted_state with a line list: spectra made with the list, a joint state whose thresholds sit
    next to the likelihoods of `params` (at the relative distances `offsets`), and those."""
    from massivedatans_amd import _lib, jointstate
    from massivedatans_amd.like import MuseSpectra
    rng = np.random.RandomState(seed)
    data = gen.muse_like(ndata, nx, lines=lines, ref=ref)
    sp = MuseSpectra(data["x"], data["y"], data["v"], lines=lines, ref=ref)
    st = jointstate.MuseJointState(sp, nlive, shelf_cap=4)
    st.init(physical(rng, nlive, lines))
    params = physical(rng, B, lines)
    L = sp.loglike_batch_lines(params, None)                       # exact kernels, [B, ndata]
    live = st.live_matrix()
    which = np.arange(ndata) % B
    off = np.asarray(offsets)[rng.randint(len(offsets), size=ndata)]
    base = L[which, np.arange(ndata)]
    thr = base + off * np.abs(base)
    live[:] = np.maximum(live, thr[None, :] + 1e6)
    live[0] = thr
    st._check(st._lib.mdns_joint_set_live(st._h, _lib.ptr(np.ascontiguousarray(live))), "mdns_joint_set_live")
    st.prepare()
    return sp, st, params, L, thr
