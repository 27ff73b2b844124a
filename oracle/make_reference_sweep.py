"""Generate tests/golden/reference_sweep.npz: the seeded sweep of tests/test_oracle.py
(test_port_vs_compiled_reference_random), with the REFERENCE's own outputs (oracle/_ref).

TEST INFRASTRUCTURE.  Run where the reference's sources are (REF in oracle/Makefile):

    make -C oracle && python oracle/make_reference_sweep.py

Inputs and outputs only (data, no reference source): the test compares the CPU oracle with
these recorded outputs on every machine, and with the compiled reference as well where
oracle/_ref is present.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from oracle.oracle import Oracle, have_reference  # noqa: E402

NTRIALS = 12
PATH = os.path.join(os.path.dirname(HERE), "tests", "golden", "reference_sweep.npz")


def sweep_inputs():
    """The trials' inputs, drawn from RandomState(7) in the test's original order."""
    rng = np.random.RandomState(7)
    trials = []
    for _ in range(NTRIALS):
        t = {}
        nd, nx = int(rng.randint(1, 70)), int(rng.randint(1, 50))
        t["x"] = np.sort(rng.uniform(400, 800, nx))
        t["yy"] = np.ascontiguousarray(rng.normal(0, 0.05, size=(nx, nd)))
        t["m"] = rng.uniform(size=nd) < rng.uniform()
        t["gauss"] = np.array([rng.uniform(0.01, 1), rng.uniform(400, 800), 10 ** rng.uniform(0, 2)])
        t["vv"] = np.ascontiguousarray(rng.uniform(0.5, 2, size=(nx, nd)) * 1e-4)
        t["yp"] = rng.uniform(0, 2, nx)
        ndim, K, M = int(rng.randint(1, 7)), int(rng.randint(2, 90)), int(rng.randint(1, 60))
        t["pts"], t["cand"] = rng.uniform(size=(K, ndim)), rng.uniform(size=(M, ndim))
        t["r"] = np.float64(rng.uniform(0.05, 0.6))
        chosen = np.zeros((K, 10))
        for b in range(10):
            chosen[rng.choice(np.arange(K), size=K, replace=True), b] = 1.
        t["chosen"] = chosen
        trials.append(t)
    return trials


def sweep_outputs(orc, t):
    """What one implementation computes for one trial (the keys the fixture stores)."""
    a, mu, sig = t["gauss"]
    out = {"gauss_out": orc.gauss_like(t["x"], t["yy"], a, mu, sig, 0.01, t["m"])}
    nd = t["yy"].shape[1]
    L = np.full(nd, -1.0)
    orc.muse_like(t["yy"], t["vv"], t["yp"], t["m"], Lout=L)
    out["muse_out"] = L
    for cm in (0, 1, 2):
        out["count%d" % cm] = orc.count_within_distance_of(t["pts"], float(t["r"]), t["cand"], cm)
    out["nn"] = np.float64(orc.most_distant_nearest_neighbor(t["pts"]))
    out["radius"] = np.float64(orc.bootstrapped_maxdistance(t["pts"], t["chosen"]))
    return out


def main():
    assert have_reference(), "oracle/_ref missing: run `make -C oracle` where the reference's sources are (REF)"
    ref = Oracle("reference")
    out = {}
    for i, t in enumerate(sweep_inputs()):
        for k, v in list(t.items()) + list(sweep_outputs(ref, t).items()):
            out["t%d_%s" % (i, k)] = v
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
