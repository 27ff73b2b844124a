#!/usr/bin/env python3
"""Device time of ONE draw chunk of a caller-defined model (mdns_backend_draw_curves[_dev]) beside the built-in
parameter chunk of the same shape (mdns_backend_draw_chunk), from the same run:

    python tools/curve_chunk_bench.py [--small]

Two shapes: 256 candidates x 10 000 spectra x 200 channels (fixed noise, the Gaussian line) and 64 x 6 250 x 4096
(scale-marginalised, the three-line template).  Per shape, HIP events on the library stream around a chunk
(mdns_event_*): the stream is idle when the first one is recorded and a chunk ends with the host polling its
mailbox, so the span between the events is the whole chunk as the stream sees it -- copies, kernels and the gaps the
host leaves between its commands.  (The kernels alone: `rocprofv3 --kernel-trace --memory-copy-trace --stats` over
this program.)  Three ways, alternating, median of the repeats:

    params         the built-in chunk: templates computed on the device from the parameters
    curves host    the same templates made in numpy, handed over as a host array (one host-to-device copy per chunk)
    curves device  the same curves already in device memory (mdns_backend_draw_curves_dev)

``copy share`` = (curves host - curves device) / curves host.  The candidates are rejected by every data set, so the
state never changes.  Synthetic spectra; prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from massivedatans_amd import _lib, gen, jointstate, sample  # noqa: E402
from massivedatans_amd.like import GaussLineSpectra, MuseSpectra  # noqa: E402

small = "--small" in sys.argv
REPEATS = 5 if small else 40


def timed(lib, fn, ev):
    _lib.check(lib.mdns_event_record(ev[0]), "event")
    fn()
    _lib.check(lib.mdns_event_record(ev[1]), "event")
    return lib.mdns_event_elapsed_ms(ev[0], ev[1]) * 1e3


def measure(lib, ways):
    ev = (lib.mdns_event_create(), lib.mdns_event_create())
    for fn in ways.values():                       # warm up every way
        for _ in range(3):
            fn()
    us = {name: [] for name in ways}
    for _ in range(REPEATS):                       # alternating
        for name, fn in ways.items():
            us[name].append(timed(lib, fn, ev))
    for e in ev:
        lib.mdns_event_destroy(e)
    return {name: {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1),
                   "max_us": round(float(np.max(v)), 1)} for name, v in us.items()}


class DeviceCurves(object):
    """Curves uploaded once; ``chunk`` scores them from device memory."""

    def __init__(self, lib, js, curves, rows):
        self.lib, self.js, self.B, self.nx = lib, js, len(curves), curves.shape[1]
        self.M = js.ndata if rows is None else len(rows)
        self.d = lib.mdns_dev_alloc(curves.nbytes)
        _lib.check(lib.mdns_h2d(self.d, _lib.ptr(curves), curves.nbytes), "h2d")
        self.accepted, self.nscored = C.c_int(0), C.c_int(0)
        self.bits = np.zeros((self.M + 63) // 64, dtype=np.uint64)

    def chunk(self):
        _lib.check(self.lib.mdns_backend_draw_begin(self.js._h, None, self.M), "begin")
        _lib.check(self.lib.mdns_backend_draw_curves_dev(self.js._h, self.d, self.nx, self.B, None, C.addressof(self.accepted),
                                                         _lib.ptr(self.bits), C.addressof(self.nscored)), "curves_dev")
        assert self.accepted.value == -1


def shape(lib, name, spectra, params_state, curve_state, params, curves):
    assert params_state.draw_params(params, None)[0] == -1 and curve_state.draw_params(np.arange(len(curves))[:, None], None)[0] == -1
    dev = DeviceCurves(lib, curve_state, curves, None)
    index = np.arange(len(curves), dtype=float)[:, None]
    res = measure(lib, {"params": lambda: params_state.draw_params(params, None),
                        "curves host": lambda: curve_state.draw_params(index, None),
                        "curves device": dev.chunk})
    host, device = res["curves host"]["median_us"], res["curves device"]["median_us"]
    res["copy share"] = round((host - device) / host, 3)
    res["shape"] = name
    print(res, flush=True)
    return res


def main():
    lib = _lib.require_device()
    rng = np.random.RandomState(1)
    out = []
    # fixed noise: B x ndata x nx = 256 x 10 000 x 200
    ndata, B, nlive = (500, 32, 20) if small else (10000, 256, 100)
    d = gen.horns(ndata)
    x = d["x"]
    spectra = GaussLineSpectra(x, d["y"], noise_level=0.01)
    cube = rng.uniform(size=(nlive, 3))
    cube[:, 0] *= 0.01
    live = sample.kernel_params(sample.priortransform_batch(cube))
    bad = sample.kernel_params(sample.priortransform_batch(np.column_stack([np.full(B, 1.0), rng.uniform(size=B), np.full(B, 1.0)])))

    def line(p):
        return np.ascontiguousarray(p[:, 0, None] * np.exp(-0.5 * ((p[:, 1, None] - x[None]) / p[:, 2, None]) ** 2))
    curves = line(bad)
    a = jointstate.GaussJointState(spectra, nlive, lambda p: p, fetch_rows=False, via_backend=True)
    table = np.vstack((curves, line(live)))
    b = jointstate.CurveJointState(spectra, nlive, lambda xs: table[xs[:, 0].astype(int)])
    a.init(live)
    b.init(np.arange(B, B + nlive, dtype=float)[:, None])
    a.prepare()
    b.prepare()
    out.append(shape(lib, "%d x %d x %d fixed noise" % (B, ndata, len(x)), spectra, a, b, bad, curves))
    a.close()
    b.close()
    spectra.close()
    # scale-marginalised: 64 x 6 250 x 4096
    ndata, nx, B, nlive = (300, 512, 8, 10) if small else (6250, 4096, 64, 40)
    x = np.linspace(4750, 9350, nx)
    v = rng.uniform(0.5, 2.0, size=(nx, ndata)) * 1e-4
    y = 1.0 + rng.normal(0, 1, size=(nx, ndata)) * np.sqrt(v)
    spectra = MuseSpectra(x, y, v)
    live = np.column_stack([np.full(nlive, -3.0), rng.uniform(0, 0.02, nlive), rng.uniform(-0.5, 0.5, nlive), np.ones(nlive), np.ones(nlive)])
    bad = np.column_stack([np.full(B, 1.0), rng.uniform(0, 0.02, B), rng.uniform(-0.5, 0.5, B), np.ones(B), np.ones(B)])
    table = np.ascontiguousarray(np.vstack((spectra.templates(bad), spectra.templates(live))))
    curves = np.ascontiguousarray(table[:B])
    a = jointstate.MuseJointState(spectra, nlive)
    b = jointstate.CurveJointState(spectra, nlive, lambda xs: table[xs[:, 0].astype(int)])
    a.init(live)
    b.init(np.arange(B, B + nlive, dtype=float)[:, None])
    a.prepare()
    b.prepare()
    out.append(shape(lib, "%d x %d x %d scale-marginalised" % (B, ndata, nx), spectra, a, b, bad, curves))
    print(json.dumps({"repeats": REPEATS, "shapes": out}))


if __name__ == "__main__":
    main()
