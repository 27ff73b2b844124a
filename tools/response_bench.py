#!/usr/bin/env python3
"""What the instrument response on the device (include/mdns.h Part 13, csrc/mdns_response.hip) costs and saves, measured
on the GPU:

    python tools/response_bench.py [fold] [chunk] [--small] [--processes N] [--out profiles/response_bench.jsonl]

Two parts, each in fresh child processes (``--child PART RESPONSE``; torch is imported first there: one HIP runtime per
process), the routes of a part alternating inside every round of a process; the parent prints and appends one JSON line
per part and response with the median over all rounds of all processes and the smallest and the largest round beside it.

Two responses, both a Gaussian line-spread function cut at 3 sigma (tests/response_support.py's shape):
``lsf60`` 1024 channels x 1100 bins, about 60 entries per row; ``lsf300`` 4096 x 2048, about 300 per row.

fold    k_response_fold alone (mdns_response_fold_batch_dev) at B = 256: device events around 64 back-to-back calls; a
        figure is a call in a stream of them.  ``bytes`` is what a call must move at least (the matrix in its device
        layout once, the curves once, the output once).
chunk   ONE Poisson draw chunk of 256 candidates x 10 000 spectra from the call to the polled outcome (host clock; the
        call is synchronous).  Routes of this build: ``device_numpy`` (a numpy model of n_in bins, the spectra fold) and
        ``device_table`` (a TableModel bound to x_in: no curve leaves the device).  Routes a caller has without Part 13,
        each scored through a response-less problem: ``numpy_dense`` (the numpy model folds with a dense ``@``),
        ``scipy_csr`` (the same with scipy.sparse; left out where scipy is not installed) and ``torch_dense`` (the model
        in torch on the device, folded with a dense fp64 matmul, read by mdns_backend_draw_curves_dev where it lies).
        Every candidate is rejected, so the state never changes.  ``numpy_model_alone`` is the numpy model by itself
        (no fold, no scoring): what the three numpy routes share.  The children run with ``OMP_WAIT_POLICY=passive`` and
        ``KMP_BLOCKTIME=0``: BLAS and torch worker threads that keep spinning after a product use up the processor time
        the process is allowed, and the stall lands on whichever route comes next.

Synthetic data from seeds.  There is no CPU path: without a device every part fails."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESPONSES = {"lsf60": (1024, 1100, 10.0), "lsf300": (4096, 2048, 50.0)}     # nx, n_in, sigma in bins
SMALL = {"lsf60": (128, 140, 3.0), "lsf300": (256, 128, 8.0)}


def spread(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2), "n": len(v)}


def make_response(name, small):
    """The line-spread function ``name`` with ``x_in``: channel j sits at bin j (n_in - 1) / (nx - 1)."""
    import numpy as np
    from massivedatans_amd.response import Response
    nx, n_in, sigma = (SMALL if small else RESPONSES)[name]
    centre = np.arange(nx) * ((n_in - 1) / (nx - 1))
    cols, vals, rowptr = [], [], [0]
    for j in range(nx):
        c = np.arange(max(0, int(np.ceil(centre[j] - 3 * sigma))), min(n_in - 1, int(np.floor(centre[j] + 3 * sigma))) + 1)
        cols.append(c)
        vals.append(np.exp(-0.5 * ((c - centre[j]) / sigma) ** 2) / (sigma * np.sqrt(2 * np.pi)) * (n_in / nx))
        rowptr.append(rowptr[-1] + len(c))
    return Response(np.array(rowptr, dtype=np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(vals), n_in,
                    x_in=np.linspace(1.0, 10.0, n_in))


def line_table(x_in):
    """A line of four widths on a continuum, tabulated on the bins themselves: candidates are (width, A)."""
    import numpy as np
    from massivedatans_amd.tablemodel import TableModel
    widths = np.array([0.2, 0.4, 0.8, 1.6])
    table = 0.3 + np.exp(-0.5 * ((x_in[None, :] - 5.0) / widths[:, None]) ** 2)
    return TableModel([widths], x_in, table, amplitude=True)


# ------------------------------------------------------------------------------------------ children -----------
def child_fold(name, small, rounds):
    import numpy as np
    from massivedatans_amd import _lib
    lib = _lib.require_device()
    resp = make_response(name, small)
    B, calls = (32, 8) if small else (256, 64)
    dr = resp.bind()
    curves = np.random.RandomState(1).uniform(size=(B, resp.n_in))
    d_c, d_o = lib.mdns_dev_alloc(curves.nbytes), lib.mdns_dev_alloc(B * resp.nx * 8)
    _lib.check(lib.mdns_h2d(d_c, _lib.ptr(curves), curves.nbytes), "h2d")
    ev = (lib.mdns_event_create(), lib.mdns_event_create())
    us = []
    for r in range(rounds + 1):                                            # (round 0 warms up)
        _lib.check(lib.mdns_event_record(ev[0]), "event")
        for _ in range(calls):
            _lib.check(lib.mdns_response_fold_batch_dev(dr.handle, d_c, resp.n_in, B, d_o, resp.nx), "mdns_response_fold_batch_dev")
        _lib.check(lib.mdns_event_record(ev[1]), "event")
        t = lib.mdns_event_elapsed_ms(ev[0], ev[1]) * 1e3 / calls
        if r:
            us.append(t)
    out = np.empty((B, resp.nx))
    _lib.check(lib.mdns_d2h(_lib.ptr(out), d_o, out.nbytes), "d2h")
    assert np.array_equal(out, resp.statement(curves))
    lens = np.diff(resp.rowptr)
    padded = int(sum(64 * lens[g:g + 64].max() for g in range(0, resp.nx, 64)))
    return {"shape": "%d x %d x %d" % (B, resp.nx, resp.n_in), "nnz": resp.nnz, "per_row": round(resp.nnz / resp.nx, 1),
            "bytes": padded * 12 + curves.nbytes + out.nbytes, "us": us}


def child_chunk(name, small, rounds):
    import torch                                                           # first: one HIP runtime per process
    torch.cuda.set_device(0)
    import numpy as np
    from massivedatans_amd import jointstate
    from massivedatans_amd.like import CountSpectra
    resp = make_response(name, small)
    ndata, B, nlive = (300, 32, 20) if small else (10000, 256, 100)
    x_in = resp.x_in
    x = np.linspace(1.0, 10.0, resp.nx)
    tm = line_table(x_in)
    rng = np.random.RandomState(2)

    def draw(n, A):
        return np.ascontiguousarray(np.column_stack((rng.uniform(0.2, 1.6, size=n), np.full(n, A))))
    fine = lambda xs: tm.statement(x_in, xs)                               # the numpy model: [B, n_in]
    R = resp.dense()
    RT = np.ascontiguousarray(R.T)
    truth = draw(ndata, 20.0)
    y = rng.poisson(fine(truth) @ RT).astype(float).T                      # [nx, ndata]
    with_r, without = CountSpectra(x, y), CountSpectra(x, y)
    with_r.set_response(resp)
    live, bad = draw(nlive, 20.0), draw(B, 1000.0)                         # fifty times too bright: nobody takes them
    d_RT = torch.from_numpy(RT).to("cuda")
    d_table = torch.from_numpy(tm.table).to("cuda")
    d_w = torch.from_numpy(tm.axes[0]).to("cuda")

    def torch_dense(xs):
        p = torch.from_numpy(xs).to("cuda")
        v = torch.clamp(p[:, 0], d_w[0], d_w[-1]).contiguous()
        i = torch.clamp(torch.searchsorted(d_w, v, right=True) - 1, 0, len(d_w) - 2)
        f = ((v - d_w[i]) / (d_w[i + 1] - d_w[i]))[:, None]
        return (p[:, 1, None] * ((1.0 - f) * d_table[i] + f * d_table[i + 1])) @ d_RT
    states = {"device_numpy": jointstate.CurveJointState(with_r, nlive, fine, ndim=2),
              "device_table": jointstate.CurveJointState(with_r, nlive, None, table=tm.bind(x_in)),
              "numpy_dense": jointstate.CurveJointState(without, nlive, lambda xs: fine(xs) @ RT, ndim=2),
              "torch_dense": jointstate.CurveJointState(without, nlive, torch_dense, ndim=2)}
    try:
        import scipy.sparse
        csr = scipy.sparse.csr_matrix((resp.vals, resp.cols, resp.rowptr), shape=(resp.nx, resp.n_in))
        states["scipy_csr"] = jointstate.CurveJointState(without, nlive, lambda xs: np.ascontiguousarray((csr @ fine(xs).T).T), ndim=2)
    except ImportError:
        pass
    assert np.allclose(torch_dense(bad).cpu().numpy(), resp.statement(fine(bad)), rtol=1e-10)
    for js in states.values():
        js.init(live)
        js.prepare()
    us = {n: [] for n in list(states) + ["numpy_model_alone"]}
    # the Python-heavy routes first, the device routes behind an untimed chunk: a device route timed right after
    # milliseconds of numpy would be timed on a GPU that had gone idle
    order = ["numpy_dense"] + (["scipy_csr"] if "scipy_csr" in states else []) + ["torch_dense", "device_numpy", "device_table"]
    for r in range(rounds + 2):                                            # (two warm-up rounds)
        t0 = time.perf_counter()
        fine(bad)
        if r >= 2:
            us["numpy_model_alone"].append((time.perf_counter() - t0) * 1e6)
        for n in order:
            if n == "torch_dense":
                states["device_table"].draw_params(bad, None)
            t0 = time.perf_counter()
            idx = states[n].draw_params(bad, None)[0]
            t = (time.perf_counter() - t0) * 1e6
            assert idx == -1
            if r >= 2:
                us[n].append(t)
    return {"shape": "%d x %d spectra x %d channels, %d bins" % (B, ndata, resp.nx, resp.n_in), "per_row": round(resp.nnz / resp.nx, 1), "us": us}


CHILDREN = {"fold": (child_fold, 10), "chunk": (child_chunk, 10)}


# ------------------------------------------------------------------------------------------ the parent ---------
def main():
    small = "--small" in sys.argv
    if "--child" in sys.argv:
        at = sys.argv.index("--child")
        fn, rounds = CHILDREN[sys.argv[at + 1]]
        print(json.dumps(fn(sys.argv[at + 2], small, 2 if small else rounds)))
        return
    processes = int(sys.argv[sys.argv.index("--processes") + 1]) if "--processes" in sys.argv else 3
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    parts = [a for a in sys.argv[1:] if a in CHILDREN] or list(CHILDREN)
    names = [a for a in sys.argv[1:] if a in RESPONSES] or list(RESPONSES)
    lines = []
    for part in parts:
        for name in names:
            got = []
            for _ in range(processes):                                     # fresh processes
                cmd = [sys.executable, os.path.abspath(__file__), "--child", part, name] + (["--small"] if small else [])
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                                     env=dict(os.environ, OMP_WAIT_POLICY="passive", KMP_BLOCKTIME="0"))
                if res.returncode != 0:
                    sys.exit("response_bench: part %s %s failed:\n%s" % (part, name, (res.stdout + res.stderr)[-3000:]))
                got.append(json.loads(res.stdout.strip().splitlines()[-1]))
            line = {"tool": "response_bench", "part": part, "response": name, "processes": processes, "small": small,
                    "shape": got[0]["shape"], "entries_per_row": got[0]["per_row"]}
            if part == "fold":
                line["us_per_call"] = spread(sum((g["us"] for g in got), []))
                line["bytes_per_call"] = got[0]["bytes"]
                line["rate_TBps"] = round(got[0]["bytes"] / (line["us_per_call"]["median"] * 1e-6) / 1e12, 3)
            else:
                for route in got[0]["us"]:
                    line[route + "_us"] = spread(sum((g["us"][route] for g in got), []))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if out_path:
        with open(out_path, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
