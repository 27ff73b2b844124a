#!/usr/bin/env python3
"""The four curve kernels on the same shapes, data and curves already on the device: the fixed-scale chi^2 with
per-pixel weights (mdns_curve_chi2_batch_dev, k_curve_rows_w), the Poisson likelihood of counts
(mdns_curve_poisson_batch_dev, k_curve_log + k_curve_rows_p) and the W statistic of counts with a background
(mdns_curve_wstat_batch_dev, k_curve_rows_b) against the fixed-noise likelihood (mdns_curve_loglike_batch_dev,
k_curve_rows):

    python tools/curve_bench.py [reps] [rounds] >> profiles/curve_bench.jsonl

Shapes (candidates x spectra x channels): 256 x 10 000 x 200 (a full chunk over the benchmark's spectra) and
32 x 128 x 64 (one workgroup: the launch itself).  Per kernel the device time of one call, from events around `reps`
calls; the kernels alternate within a round, the median over the rounds is reported with its spread and the ratios.
The Poisson call is two launches, timed together; their shares come from a kernel trace of this program
(profiles/README.md).  One JSON line per shape.

    python tools/curve_bench.py --torch [reps] [rounds] >> profiles/curve_bench.jsonl

sets, at 32 x 1000 x 200, the W kernel against what a caller could write without it: the statement of include/mdns.h
Part 11 as elementwise float64 torch on the device over [B, M, nx] (`torch_wstat` below; its temporaries fit at that
shape), timed by torch's events on torch's stream, alternating with the kernel in the same rounds.  A run of its own
because torch has to be imported before the library is loaded (one HIP runtime per process)."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from massivedatans_amd import _lib, gen
from massivedatans_amd.like import CountSpectra, WeightedSpectra

SHAPES = ((256, 10000, 200), (32, 128, 64))
POISSON = "k_curve_log+k_curve_rows_p"
WSTAT = "k_curve_rows_b"
KERNELS = ("k_curve_rows", "k_curve_rows_w", POISSON, WSTAT)
TORCH_SHAPE = (32, 1000, 200)


def count_case(x, nx, ndata, rng):
    """Counts of a few per pixel at exposures in [0.5, 2] over a background of about two per pixel, seen in a background
    region of exposure [2, 6]: (y, e, b, g) [nx, ndata]."""
    e, g = rng.uniform(0.5, 2.0, size=(nx, ndata)), rng.uniform(2.0, 6.0, size=(nx, ndata))
    return rng.poisson(3.0 * e).astype(float), e, rng.poisson(2.0 * e).astype(float), rng.poisson(2.0 * g).astype(float), g


def torch_wstat(c, n, e, b, g, Kw):
    """The statement as a caller would write it: c [B, 1, nx] >= 0, the data [1, M, nx], Kw [M] -> L [B, M]."""
    import torch
    tiny = torch.finfo(torch.float64).tiny
    T, N = e + g, n + b
    a = N - T * c
    d = torch.sqrt(a * a + 4 * T * b * c)
    f = torch.where(a >= 0, (a + d) / (2 * T), 2 * b * c / (d - a))
    s = c + f
    return (n * torch.log(s.clamp_min(tiny)) + b * torch.log(f.clamp_min(tiny)) - e * s - g * f).sum(dim=2) + Kw


def main():
    args = [a for a in sys.argv[1:] if a != "--torch"]
    reps = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 5
    if "--torch" in sys.argv[1:]:
        import torch                                       # first: one HIP runtime per process
        torch.cuda.set_device(0)
        return against_torch(_lib.require_device(), reps, rounds)
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
        n_src, exposure, n_bg, b_bg, g_bg = count_case(d["x"], nx, ndata, rng)
        counts = CountSpectra(d["x"][:nx], n_src, exposure)
        both = CountSpectra(d["x"][:nx], n_src + n_bg, exposure, b_bg, g_bg)
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
            elif name == POISSON:
                _lib.check(lib.mdns_curve_poisson_batch_dev(counts.handle, d_p, nx, B, None, ndata, d_o), "mdns_curve_poisson_batch_dev")
            else:
                _lib.check(lib.mdns_curve_wstat_batch_dev(both.handle, d_p, nx, B, None, ndata, d_o), "mdns_curve_wstat_batch_dev")

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
                          "ratio_p_to_w": round(us[POISSON] / us["k_curve_rows_w"], 3),
                          "ratio_b_to_p": round(us[WSTAT] / us[POISSON], 3)}))
        lib.mdns_event_destroy(e0); lib.mdns_event_destroy(e1)
        for p in (d_c, d_p, d_o):
            lib.mdns_dev_free(p)
        sp.close()
        counts.close()
        both.close()


def against_torch(lib, reps, rounds):
    import torch
    from massivedatans_amd.like import background_pixels
    B, ndata, nx = TORCH_SHAPE
    rng = np.random.RandomState(B)
    x = np.linspace(400.0, 800.0, nx)
    n_src, e, n_bg, b, g = count_case(x, nx, ndata, rng)
    y = n_src + n_bg
    both = CountSpectra(x, y, e, b, g)
    rates = rng.uniform(0.0, 6.0, size=(B, nx))
    Kw = background_pixels(y, e, b, g)[5]
    dev = torch.device("cuda")
    t_c = torch.tensor(rates, device=dev)[:, None, :]
    t_n, t_e, t_b, t_g = (torch.tensor(np.ascontiguousarray(a.T), device=dev)[None] for a in (y, e, b, g))
    t_K = torch.tensor(Kw, device=dev)
    d_p, d_o = lib.mdns_dev_alloc(rates.nbytes), lib.mdns_dev_alloc(B * ndata * 8)
    if not d_p or not d_o:
        raise SystemExit("mdns_dev_alloc failed: " + _lib.last_error())
    _lib.check(lib.mdns_h2d(d_p, _lib.ptr(rates), rates.nbytes), "mdns_h2d")
    got = np.empty((B, ndata))
    _lib.check(lib.mdns_curve_wstat_batch_dev(both.handle, d_p, nx, B, None, ndata, d_o), "mdns_curve_wstat_batch_dev")
    _lib.check(lib.mdns_d2h(_lib.ptr(got), d_o, got.nbytes), "mdns_d2h")
    want = torch_wstat(t_c, t_n, t_e, t_b, t_g, t_K).cpu().numpy()
    if not np.allclose(got, want, rtol=1e-10, atol=1e-8):       # (the two time the same computation)
        raise SystemExit("the torch statement and the kernel disagree: %g" % np.abs(got - want).max())
    e0, e1 = lib.mdns_event_create(), lib.mdns_event_create()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {WSTAT: [], "torch_elementwise": []}
    for rnd in range(rounds + 1):
        lib.mdns_event_record(e0)
        for _ in range(reps):
            _lib.check(lib.mdns_curve_wstat_batch_dev(both.handle, d_p, nx, B, None, ndata, d_o), "mdns_curve_wstat_batch_dev")
        lib.mdns_event_record(e1)
        ms = lib.mdns_event_elapsed_ms(e0, e1)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(reps):
            torch_wstat(t_c, t_n, t_e, t_b, t_g, t_K)
        t1.record()
        torch.cuda.synchronize()
        if rnd:
            times[WSTAT].append(ms * 1e3 / reps)
            times["torch_elementwise"].append(t0.elapsed_time(t1) * 1e3 / reps)
    us = {name: float(np.median(v)) for name, v in times.items()}
    print(json.dumps({"B": B, "ndata": ndata, "nx": nx, "reps": reps, "rounds": rounds,
                      "us_per_call": {name: round(v, 2) for name, v in us.items()},
                      "spread_us": {name: [round(min(v), 2), round(max(v), 2)] for name, v in times.items()},
                      "ratio_b_to_torch": round(us[WSTAT] / us["torch_elementwise"], 4)}))
    lib.mdns_event_destroy(e0); lib.mdns_event_destroy(e1)
    lib.mdns_dev_free(d_p); lib.mdns_dev_free(d_o)
    both.close()


if __name__ == "__main__":
    main()
