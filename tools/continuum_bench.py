#!/usr/bin/env python3
"""The scale-marginalised scoring with a per-spectrum polynomial continuum of P terms against K2 without one (P = 0,
the exact row kernels: mdns_muse_filter_mode(0)), on templates that are on the device already:

    python tools/continuum_bench.py [reps] [rounds]

Shapes: 64 candidates x 6250 spectra x 4096 channels (one GPU's share of BASELINE configs[4]) and 8 x 400 x 4096 (a
late draw chunk).  Per setting the device time of one mdns_muse_loglike_batch_dev call (template padding + scoring),
from events around `reps` calls; the settings alternate within a round, the median over the rounds is reported, with
the P/0 ratios.  One JSON line."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from massivedatans_amd import _lib, gen, musefuse
from massivedatans_amd.like import MuseSpectra

SHAPES = ((64, 6250, 4096), (8, 400, 4096))
SETTINGS = (0, 1, 2, 4)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lib = _lib.require_device()
    lib.mdns_muse_filter_mode(0)
    out = {"reps": reps, "rounds": rounds, "shapes": []}
    for B, ndata, nx in SHAPES:
        d = gen.muse_like(ndata, nx, continuum=2)
        sp = MuseSpectra(d["x"], d["y"], d["v"])
        rng = np.random.RandomState(B)
        templates = np.ascontiguousarray([gen.muse_template(d["x"], p) for p in musefuse.priortransform_batch(rng.uniform(size=(B, 5)))])
        d_t, d_o = lib.mdns_dev_alloc(templates.nbytes), lib.mdns_dev_alloc(B * ndata * 8)
        if not d_t or not d_o:
            raise SystemExit("mdns_dev_alloc failed: " + _lib.last_error())
        _lib.check(lib.mdns_h2d(d_t, _lib.ptr(templates), templates.nbytes), "mdns_h2d")
        e0, e1 = lib.mdns_event_create(), lib.mdns_event_create()
        times = {P: [] for P in SETTINGS}
        kernels = {}

        def call():
            _lib.check(lib.mdns_muse_loglike_batch_dev(sp.handle, d_t, B, None, ndata, d_o), "mdns_muse_loglike_batch_dev")

        for rnd in range(rounds + 1):                      # (round 0 warms every setting up and is not kept)
            for P in SETTINGS:
                _lib.check(lib.mdns_spectra_set_continuum(sp.handle, P), "mdns_spectra_set_continuum")
                call()
                lib.mdns_event_record(e0)
                for _ in range(reps):
                    call()
                lib.mdns_event_record(e1)
                ms = lib.mdns_event_elapsed_ms(e0, e1)
                kernels[P] = (lib.mdns_profile_kernel(1) or b"").decode()
                if rnd:
                    times[P].append(ms * 1e3 / reps)
        us = {P: float(np.median(times[P])) for P in SETTINGS}
        out["shapes"].append({"B": B, "ndata": ndata, "nx": nx,
                              "us_per_call": {str(P): round(us[P], 2) for P in SETTINGS},
                              "spread_us": {str(P): [round(min(times[P]), 2), round(max(times[P]), 2)] for P in SETTINGS},
                              "ratio_to_P0": {str(P): round(us[P] / us[0], 3) for P in SETTINGS if P},
                              "kernel": {str(P): kernels[P] for P in SETTINGS}})
        lib.mdns_event_destroy(e0); lib.mdns_event_destroy(e1)
        lib.mdns_dev_free(d_t); lib.mdns_dev_free(d_o)
        sp.close()
    lib.mdns_muse_filter_mode(-1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
