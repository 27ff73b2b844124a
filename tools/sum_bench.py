#!/usr/bin/env python3
"""What the sum model on the device (include/mdns.h Part 14, csrc/mdns_sum.hip) costs and saves, measured on the GPU:

    python tools/sum_bench.py [a] [b] [--small] [--processes N] [--out profiles/sum_bench.jsonl]

One Poisson draw chunk of 256 candidates x 10 000 spectra through the 1024 x 1100 response of tools/response_bench.py
(about 59 entries per row), from the call to the polled outcome (host clock; the call is synchronous), per model in
fresh child processes (``--child MODEL``; torch is imported first there: one HIP runtime per process), the routes
alternating inside every round of a process; the parent prints and appends one JSON line per model with the median over
all rounds of all processes and the smallest and the largest round beside it.

a   ``att x (power law + Gaussian line)``: ``device_sum`` (a SumModel bound to x_in: parameters go in, no curve leaves
    the device), ``torch`` (the same physics in torch on the device, read by mdns_backend_draw_curves_dev where it lies)
    and ``numpy`` (the same physics in numpy; the curves cross to the device).
b   ``att x (power law + line) + table``: ``device_sum`` against ``fetch_and_add``, what a caller had before: a Python
    model that fetches ``DeviceTable.curves`` to the host and adds the numpy parts.

The comparators are routes that exist without Part 14.  ``curves_alone_us`` is mdns_sum_curves_batch_dev by itself at
B = 256 (device events around 64 back-to-back calls: a call in a stream of them); ``launches`` the kernels it starts.
Every candidate is rejected, so the state never changes.  The children run with ``OMP_WAIT_POLICY=passive`` and
``KMP_BLOCKTIME=0`` (tools/response_bench.py says why).

Synthetic data from seeds.  There is no CPU path: without a device every part fails."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODELS = ("a", "b")


def spread(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2), "n": len(v)}


def child(which, small, rounds):
    import torch                                                           # first: one HIP runtime per process
    torch.cuda.set_device(0)
    import numpy as np
    from massivedatans_amd import _lib, jointstate
    from massivedatans_amd.like import CountSpectra
    from massivedatans_amd.summodel import GaussianLine, PowerLaw, SumModel
    from response_bench import line_table, make_response
    lib = _lib.require_device()
    resp = make_response("lsf60", small)
    ndata, B, nlive, calls = (300, 32, 20, 8) if small else (10000, 256, 100, 64)
    x_in = resp.x_in
    x = np.linspace(1.0, 10.0, resp.nx)
    att = -0.4 * (x_in[0] / x_in) ** 2.5                                   # an absorber: strongest at the low end
    tm = line_table(x_in)                                                  # candidates (width, A)
    lx = np.log10(x_in / 1.0)
    rng = np.random.RandomState(2)

    def draw(n, scale):
        cols = [np.log10(scale) + rng.uniform(0.0, 0.3, size=n), rng.uniform(1.0, 2.5, size=n),              # logA, G
                scale * rng.uniform(0.5, 2.0, size=n), rng.uniform(4.0, 7.0, size=n), rng.uniform(0.1, 0.5, size=n)]   # A, mu, sigma
        if which == "b":
            cols += [rng.uniform(0.2, 1.6, size=n), scale * np.ones(n)]
        return np.ascontiguousarray(np.column_stack(cols + [rng.uniform(0.0, 2.0, size=n)]))

    def analytic(xs):
        """att x (power law + line) in numpy on the bins: [B, n_in]."""
        pl = 10 ** (xs[:, 0, None] - xs[:, 1, None] * lx[None, :])
        line = xs[:, 2, None] * np.exp(-0.5 * ((x_in[None, :] - xs[:, 3, None]) / xs[:, 4, None]) ** 2)
        return (pl + line) * 10 ** (att[None, :] * xs[:, -1, None])
    comps = [PowerLaw(x0=1.0), GaussianLine()] + ([tm] if which == "b" else [])
    sm = SumModel(comps, attenuation=att, unattenuated=[2] if which == "b" else [])
    dsum = sm.bind(x_in)
    truth = draw(ndata, 20.0)
    y = rng.poisson(sm.statement(x_in, truth) @ np.ascontiguousarray(resp.dense().T)).astype(float).T   # [nx, ndata]
    spectra = CountSpectra(x, y)
    spectra.set_response(resp)
    live, bad = draw(nlive, 20.0), draw(B, 1000.0)                         # fifty times too bright: nobody takes them
    states = {"device_sum": jointstate.CurveJointState(spectra, nlive, None, table=dsum)}
    if which == "a":
        d_lx, d_x, d_att = (torch.from_numpy(a).to("cuda") for a in (lx, x_in, att))

        def in_torch(xs):
            p = torch.from_numpy(xs).to("cuda")
            pl = 10 ** (p[:, 0, None] - p[:, 1, None] * d_lx[None, :])
            line = p[:, 2, None] * torch.exp(-0.5 * ((d_x[None, :] - p[:, 3, None]) / p[:, 4, None]) ** 2)
            return (pl + line) * 10 ** (d_att[None, :] * p[:, -1, None])
        assert np.allclose(in_torch(bad).cpu().numpy(), sm.statement(x_in, bad), rtol=1e-10)
        states["torch"] = jointstate.CurveJointState(spectra, nlive, in_torch, ndim=sm.ndim)
        states["numpy"] = jointstate.CurveJointState(spectra, nlive, analytic, ndim=sm.ndim)
        order = ["numpy", "torch", "device_sum"]
    else:
        table = tm.bind(x_in)
        states["fetch_and_add"] = jointstate.CurveJointState(spectra, nlive, lambda xs: analytic(xs) + table.curves(xs[:, 5:7]), ndim=sm.ndim)
        order = ["fetch_and_add", "device_sum"]
    assert np.allclose(analytic(bad) + (tm.statement(x_in, bad[:, 5:7]) if which == "b" else 0.0), sm.statement(x_in, bad), rtol=1e-10)
    for js in states.values():
        js.init(live)
        js.prepare()
    us = {n: [] for n in order}
    # the Python-heavy route first, the device routes behind an untimed chunk: a device route timed right after
    # milliseconds of numpy would be timed on a GPU that had gone idle
    for r in range(rounds + 2):                                            # (two warm-up rounds)
        for n in order:
            if n == order[1]:
                states["device_sum"].draw_params(bad, None)
            t0 = time.perf_counter()
            idx = states[n].draw_params(bad, None)[0]
            t = (time.perf_counter() - t0) * 1e6
            assert idx == -1
            if r >= 2:
                us[n].append(t)
    # mdns_sum_curves_batch_dev alone
    d_p, d_o = lib.mdns_dev_alloc(bad.nbytes), lib.mdns_dev_alloc(B * resp.n_in * 8)
    _lib.check(lib.mdns_h2d(d_p, _lib.ptr(bad), bad.nbytes), "h2d")
    ev = (lib.mdns_event_create(), lib.mdns_event_create())
    alone = []
    for r in range(rounds + 1):                                            # (round 0 warms up)
        _lib.check(lib.mdns_event_record(ev[0]), "event")
        for _ in range(calls):
            _lib.check(lib.mdns_sum_curves_batch_dev(dsum.handle, d_p, B, d_o, resp.n_in), "mdns_sum_curves_batch_dev")
        _lib.check(lib.mdns_event_record(ev[1]), "event")
        t = lib.mdns_event_elapsed_ms(ev[0], ev[1]) * 1e3 / calls
        if r:
            alone.append(t)
    out = np.empty((B, resp.n_in))
    _lib.check(lib.mdns_d2h(_lib.ptr(out), d_o, out.nbytes), "d2h")
    assert np.array_equal(out, sm.statement(x_in, bad))
    return {"shape": "%d x %d spectra x %d channels, %d bins" % (B, ndata, resp.nx, resp.n_in), "per_row": round(resp.nnz / resp.nx, 1),
            "model": "att x (power law + line)" + (" + table" if which == "b" else ""), "launches": 2 if which == "b" else 1,
            "us": us, "alone": alone}


def main():
    small = "--small" in sys.argv
    if "--child" in sys.argv:
        print(json.dumps(child(sys.argv[sys.argv.index("--child") + 1], small, 2 if small else 10)))
        return
    processes = int(sys.argv[sys.argv.index("--processes") + 1]) if "--processes" in sys.argv else 3
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for which in [a for a in sys.argv[1:] if a in MODELS] or list(MODELS):
        got = []
        for _ in range(processes):                                         # fresh processes
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + (["--small"] if small else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                                 env=dict(os.environ, OMP_WAIT_POLICY="passive", KMP_BLOCKTIME="0"))
            if res.returncode != 0:
                sys.exit("sum_bench: model %s failed:\n%s" % (which, (res.stdout + res.stderr)[-3000:]))
            got.append(json.loads(res.stdout.strip().splitlines()[-1]))
        line = {"tool": "sum_bench", "model": got[0]["model"], "processes": processes, "small": small, "shape": got[0]["shape"],
                "entries_per_row": got[0]["per_row"], "launches": got[0]["launches"]}
        for route in got[0]["us"]:
            line[route + "_us"] = spread(sum((g["us"][route] for g in got), []))
        line["curves_alone_us"] = spread(sum((g["alone"] for g in got), []))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if out_path:
        with open(out_path, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
