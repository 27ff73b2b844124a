#!/usr/bin/env python3
"""The three curve kernels on the same shapes, data and curves already on the device: the fixed-scale chi^2 with
per-pixel weights (mdns_curve_chi2_batch_dev, k_curve_rows_w) and the Poisson likelihood of counts
(mdns_curve_poisson_batch_dev, k_curve_log + k_curve_rows_p) against the fixed-noise likelihood
(mdns_curve_loglike_batch_dev, k_curve_rows):

    python tools/curve_bench.py [reps] [rounds] >> profiles/curve_bench.jsonl

Shapes (candidates x spectra x channels): 256 x 10 000 x 200 (a full chunk over the benchmark's spectra) and
32 x 128 x 64 (one workgroup: the launch itself).  Per kernel the device time of one call, from events around `reps`
calls; the kernels alternate within a round, the median over the rounds is reported with its spread and the ratios.
The Poisson call is two launches, timed together; their shares come from a kernel trace of this program
(profiles/README.md).  One JSON line per shape."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from massivedatans_amd import _lib, gen
from massivedatans_amd.like import CountSpectra, WeightedSpectra

SHAPES = ((256, 10000, 200), (32, 128, 64))
POISSON = "k_curve_log+k_curve_rows_p"
KERNELS = ("k_curve_rows", "k_curve_rows_w", POISSON)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lib = _lib.require_device()
    for B, ndata, nx in SHAPES:
        d = gen.horns(ndata)
        rng = np.random.RandomState(B)
        y = np.ascontiguousarray(d["y"][:nx])
        sigma = 0.01 * (1 + 3 * rng.uniform(size=y.shape))
        sp = WeightedSpectra(d["x"][:nx], y, sigma ** 2)
        curves = rng.uniform(-0.1, 0.3, size=(B, nx))
        # counts of a few per pixel at exposures in [0.5, 2], rates >= 0: what the kernels compute does not depend on
        # the values, the logarithm's time on nothing but their count
        exposure = rng.uniform(0.5, 2.0, size=y.shape)
        counts = CountSpectra(d["x"][:nx], rng.poisson(3.0 * exposure).astype(float), exposure)
        rates = np.abs(curves) * 20
        d_c, d_p, d_o = (lib.mdns_dev_alloc(n) for n in (curves.nbytes, rates.nbytes, B * ndata * 8))
        if not d_c or not d_p or not d_o:
            raise SystemExit("mdns_dev_alloc failed: " + _lib.last_error())
        _lib.check(lib.mdns_h2d(d_c, _lib.ptr(curves), curves.nbytes), "mdns_h2d")
        _lib.check(lib.mdns_h2d(d_p, _lib.ptr(rates), rates.nbytes), "mdns_h2d")
        e0, e1 = lib.mdns_event_create(), lib.mdns_event_create()

        def call(name):
            if name == "k_curve_rows":
                _lib.check(lib.mdns_curve_loglike_batch_dev(sp.handle, d_c, nx, B, 0.01, None, ndata, d_o), "mdns_curve_loglike_batch_dev")
            elif name == "k_curve_rows_w":
                _lib.check(lib.mdns_curve_chi2_batch_dev(sp.handle, d_c, nx, B, None, ndata, d_o), "mdns_curve_chi2_batch_dev")
            else:
                _lib.check(lib.mdns_curve_poisson_batch_dev(counts.handle, d_p, nx, B, None, ndata, d_o), "mdns_curve_poisson_batch_dev")

        times = {name: [] for name in KERNELS}
        for rnd in range(rounds + 1):                      # (round 0 warms all up and is not kept)
            for name in KERNELS:
                call(name)
                lib.mdns_event_record(e0)
                for _ in range(reps):
                    call(name)
                lib.mdns_event_record(e1)
                ms = lib.mdns_event_elapsed_ms(e0, e1)
                if rnd:
                    times[name].append(ms * 1e3 / reps)
        us = {name: float(np.median(times[name])) for name in KERNELS}
        print(json.dumps({"B": B, "ndata": ndata, "nx": nx, "reps": reps, "rounds": rounds,
                          "us_per_call": {name: round(us[name], 2) for name in KERNELS},
                          "spread_us": {name: [round(min(times[name]), 2), round(max(times[name]), 2)] for name in KERNELS},
                          "ratio_w_to_fixed": round(us["k_curve_rows_w"] / us["k_curve_rows"], 3),
                          "ratio_p_to_fixed": round(us[POISSON] / us["k_curve_rows"], 3),
                          "ratio_p_to_w": round(us[POISSON] / us["k_curve_rows_w"], 3)}))
        lib.mdns_event_destroy(e0); lib.mdns_event_destroy(e1)
        for p in (d_c, d_p, d_o):
            lib.mdns_dev_free(p)
        sp.close()
        counts.close()


if __name__ == "__main__":
    main()
