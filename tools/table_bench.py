#!/usr/bin/env python3
"""What the table model (include/mdns.h Part 12, csrc/mdns_table.hip) costs and saves, measured on the GPU:

    python tools/table_bench.py [kernel] [chunk] [run] [los] [--small] [--processes N] [--out profiles/table_bench.jsonl]

Four parts, each in fresh child processes (``--child PART``; torch is imported first there: one HIP runtime per
process), the competitors of a part alternating inside every round of a process; the parent prints and appends one JSON
line per part with the median over all rounds of all processes and the spread (min, max) beside it.

kernel  k_table_curves alone (mdns_table_curves_batch_dev) at B = 256, nx = 200, d = 3: a 20 x 20 x 10 x 2000 table
        (64 MB: inside the Infinity Cache) and a 60 x 60 x 10 x 2000 one (576 MB: past it).  Device events around 64
        back-to-back calls that go twice through 32 different batches of candidates (so that the large table's windows
        do not simply stay cached from call to call); a figure is a call in a stream of them.  ``bytes`` is what a call
        must move on average: per candidate and corner the window of its row between the first and the last knot its
        channels read (in 128-byte lines), plus the output; ``rate`` = bytes / time, ``share`` of the gather rate
        MI355X reaches on random rows of a table of that size (8.6 TB/s inside the Infinity Cache, 6.0 TB/s from HBM).
chunk   ONE draw chunk of 256 candidates x 10 000 spectra x 200 channels from the call to the polled outcome (host
        clock; the call is synchronous), three routes: ``table`` (mdns_backend_draw_table), ``numpy`` (the vectorised
        TableModel.statement as the model: mdns_backend_draw_curves) and ``torch`` (the same interpolation in torch on
        the device: mdns_backend_draw_curves_dev reads the tensor where it lies).  Every candidate is rejected, so the
        state never changes.
run     wall time of sample.run_model over 64 spectra x 200 channels with the TableModel against the same seed with
        its statement as a numpy model (identical results are asserted).

los     the line-of-sight routes (mdns_table_create_los) on the shapes above -- the 20 x 20 x 10 x 2000 table, B = 256,
        nx = 200, 10 000 spectra: ``plain`` (z, A: k_table_curves), ``E`` (+ extinction: k_table_los_gather), ``Es8`` and
        ``Es64`` (+ broadening with windows of about +-8 and +-64 knots at the middle of the grid: the three k_table_los
        stages).  ``kernel_us``: the curves alone, as in ``kernel`` (events around 64 calls over 32 batches);
        ``chunk_us``: one draw chunk as in ``chunk``, and beside the three new routes the same model through the Python
        route (its numpy statement as the model: ``numpy_E``, ``numpy_Es8``, ``numpy_Es64``).  ``windows``: the knots in
        the window of the middle knot, and in the longest window of the grid.

Synthetic data from seeds.  There is no CPU path: without a device every part fails."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATHER_RATE = {"cache": 8.6e12, "hbm": 6.0e12}        # bytes/s, random rows gathered: inside the Infinity Cache / from HBM


def spread(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2), "n": len(v)}


def big_model(lengths, nw, seed):
    import numpy as np
    from massivedatans_amd.tablemodel import TableModel
    rng = np.random.RandomState(seed)
    axes = [np.sort(rng.uniform(0, 1, size=n)) + np.arange(n) for n in lengths]
    grid = np.cumsum(rng.uniform(0.5, 1.5, size=nw)) + 100.0        # (x / (1 + z) stays on it for z <= 0.5)
    table = 1.0 + rng.uniform(0, 1, size=tuple(lengths) + (nw,))
    return TableModel(axes, grid, table, redshift=True, amplitude=True)


def params_of(tm, rng, B, amplitude):
    import numpy as np
    cols = [rng.uniform(a[0], a[-1], size=B) for a in tm.axes] + [rng.uniform(0, 0.5, size=B), np.full(B, amplitude)]
    return np.ascontiguousarray(np.column_stack(cols))


def window_bytes(tm, x, xs):
    """Bytes of table a call must read (whole 128-byte lines of every corner row's window) and write."""
    import numpy as np
    u = np.clip(x[None, :] / (1.0 + xs[:, tm.d, None]), tm.grid[0], tm.grid[-1])
    k = np.clip(np.searchsorted(tm.grid, u, side="right") - 1, 0, len(tm.grid) - 2)
    first, last = k.min(axis=1) * 8, (k.max(axis=1) + 2) * 8
    lines = (last + 127) // 128 - first // 128
    return int((lines * 128).sum() * 2 ** tm.d + xs.shape[0] * len(x) * 8)


# ------------------------------------------------------------------------------------------ children -----------
def child_kernel(small, rounds):
    import numpy as np
    from massivedatans_amd import _lib
    lib = _lib.require_device()
    B, nx, calls, SETS = 256, 200, 64, 32
    shapes = {"cache": ([6, 6, 4], 500) if small else ([20, 20, 10], 2000), "hbm": ([8, 8, 4], 500) if small else ([60, 60, 10], 2000)}
    out, state = {}, {}
    for name, (lengths, nw) in shapes.items():
        tm = big_model(lengths, nw, seed=len(name))
        x = np.linspace(tm.grid[0] * 1.5, tm.grid[-1], nx)
        # SETS different batches of candidates, one after the other: their windows together (32 x 27 MB, over four fifths of the large table's rows) are more than
        # the Infinity Cache holds, so what a call of the large table reads was evicted since it was last read
        xs = params_of(tm, np.random.RandomState(1), SETS * B, 1.0)
        table = tm.bind(x)
        d_p, d_o = lib.mdns_dev_alloc(xs.nbytes), lib.mdns_dev_alloc(B * nx * 8)
        _lib.check(lib.mdns_h2d(d_p, _lib.ptr(xs), xs.nbytes), "h2d")
        state[name] = (tm, table, d_p, d_o, window_bytes(tm, x, xs) // SETS, [])
    ev = (lib.mdns_event_create(), lib.mdns_event_create())
    for r in range(rounds + 1):                                            # (round 0 warms up)
        for name, (tm, table, d_p, d_o, nbytes, us) in state.items():
            _lib.check(lib.mdns_event_record(ev[0]), "event")
            for i in range(calls):
                _lib.check(lib.mdns_table_curves_batch_dev(table.handle, d_p + (i % SETS) * B * tm.ndim * 8, B, d_o, nx),
                           "mdns_table_curves_batch_dev")
            _lib.check(lib.mdns_event_record(ev[1]), "event")
            t = lib.mdns_event_elapsed_ms(ev[0], ev[1]) * 1e3 / calls
            if r:
                us.append(t)
    for name, (tm, table, d_p, d_o, nbytes, us) in state.items():
        out[name] = {"table_MB": round(tm.table.nbytes / 1e6, 1), "bytes": nbytes, "us": us}
    return out


def torch_statement(tm, x, torch):
    """The statement's interpolation written in torch on the device: xs (numpy) -> float64 tensor [B, nx] on the GPU."""
    dev = torch.device("cuda")
    axes = [torch.from_numpy(a).to(dev) for a in tm.axes]
    grid, rows, xd = torch.from_numpy(tm.grid).to(dev), torch.from_numpy(tm.table.reshape(-1, len(tm.grid))).to(dev), torch.from_numpy(x).to(dev)
    strides, s = [], 1
    for a in reversed(tm.axes):
        strides.insert(0, s)
        s *= len(a)

    def model(xs):
        p = torch.from_numpy(xs).to(dev)
        B, d = p.shape[0], tm.d
        w = torch.ones((B, 1 << d), dtype=torch.float64, device=dev)
        row = torch.zeros((B, 1 << d), dtype=torch.int64, device=dev)
        for a, axis in enumerate(axes):
            v = torch.minimum(torch.maximum(p[:, a], axis[0]), axis[-1]).contiguous()
            i = torch.clamp(torch.searchsorted(axis, v, right=True) - 1, 0, len(axis) - 2)
            f = (v - axis[i]) / (axis[i + 1] - axis[i])
            for c in range(1 << d):
                bit = (c >> a) & 1
                w[:, c] = w[:, c] * (f if bit else 1.0 - f)
                row[:, c] += (i + bit) * strides[a]
        u = torch.minimum(torch.maximum(xd[None, :] / (1.0 + p[:, d, None]), grid[0]), grid[-1]).contiguous()
        k = torch.clamp(torch.searchsorted(grid, u, right=True) - 1, 0, len(grid) - 2)
        g0 = grid[k]
        t = (u - g0) / (grid[k + 1] - g0)
        acc = torch.zeros_like(u)
        for c in range(1 << d):
            lo, hi = rows[row[:, c, None], k], rows[row[:, c, None], k + 1]
            acc = acc + w[:, c, None] * (lo + t * (hi - lo))
        return p[:, -1, None] * acc
    return model


def child_chunk(small, rounds):
    import torch                                                           # first: one HIP runtime per process
    torch.cuda.set_device(0)
    import numpy as np
    from massivedatans_amd import jointstate
    from massivedatans_amd.like import GaussLineSpectra
    ndata, B, nlive, nx = (500, 32, 20, 200) if small else (10000, 256, 100, 200)
    tm = big_model([6, 6, 4] if small else [20, 20, 10], 500 if small else 2000, seed=5)
    x = np.linspace(tm.grid[0] * 1.5, tm.grid[-1], nx)
    rng = np.random.RandomState(2)
    truth = params_of(tm, rng, ndata, 1.0)
    y = np.ascontiguousarray(tm.statement(x, truth).T + 0.05 * rng.normal(size=(nx, ndata)))
    spectra = GaussLineSpectra(x, y, noise_level=0.05)
    live = params_of(tm, rng, nlive, 1.0)
    bad = params_of(tm, rng, B, 50.0)                                      # fifty times too bright: nobody takes them
    table = tm.bind(x)
    torch_model = torch_statement(tm, x, torch)
    with np.errstate(all="ignore"):
        assert np.allclose(torch_model(bad).cpu().numpy(), tm.statement(x, bad), rtol=1e-12)
    states = {"table": jointstate.CurveJointState(spectra, nlive, None, table=table),
              "numpy": jointstate.CurveJointState(spectra, nlive, lambda xs: tm.statement(x, xs), ndim=tm.ndim),
              "torch": jointstate.CurveJointState(spectra, nlive, torch_model, ndim=tm.ndim)}
    for js in states.values():
        js.init(live)
        js.prepare()
    us = {name: [] for name in states}
    for r in range(rounds + 2):                                            # (two warm-up rounds)
        for name, js in states.items():
            t0 = time.perf_counter()
            idx = js.draw_params(bad, None)[0]
            t = (time.perf_counter() - t0) * 1e6
            assert idx == -1
            if r >= 2:
                us[name].append(t)
    return {"shape": "%d x %d x %d" % (B, ndata, nx), "us": us}


def child_run(small, rounds):
    import numpy as np
    from massivedatans_amd import problem, sample
    ndata, nx, nlive, cap = (16, 64, 30, 60) if small else (64, 200, 100, 400)
    tm = big_model([5, 7, 3], 500 if small else 2000, seed=7)
    x = np.linspace(tm.grid[0] * 1.5, tm.grid[-1], nx)
    rng = np.random.RandomState(3)
    lo = np.array([a[0] for a in tm.axes] + [0.0, 0.5])
    hi = np.array([a[-1] for a in tm.axes] + [0.3, 2.0])
    prior = lambda us: lo + (hi - lo) * np.asarray(us, dtype=float)
    truth = prior(rng.uniform(0.2, 0.8, size=(ndata, tm.ndim)))
    y = np.ascontiguousarray(tm.statement(x, truth).T + 0.05 * rng.normal(size=(nx, ndata)))
    seconds, outcome = {"table": [], "numpy": []}, {}
    for r in range(rounds + 1):                                            # (round 0 warms up)
        for name, model in (("table", tm), ("numpy", lambda xs: tm.statement(x, xs))):
            p = problem.CurveProblem(x, y, model, prior, tm.ndim, noise_level=0.05)
            with np.errstate(all="ignore"):
                results, sampler, _, took = sample.run_model(p, nlive_points=nlive, max_samples=cap, use_graph=False, seed=1)
            outcome[name] = (results["logZ"], int(sampler.ndraws))
            sampler.joint.close()
            p.backend.close()
            if r:
                seconds[name].append(took * 1e3)
        assert np.array_equal(outcome["table"][0], outcome["numpy"][0]) and outcome["table"][1] == outcome["numpy"][1]
    return {"shape": "%d spectra x %d channels, %d live points, %d samples" % (ndata, nx, nlive, cap), "ndraws": outcome["table"][1],
            "ms": seconds}


def child_los(small, rounds):
    import numpy as np
    from massivedatans_amd import _lib, jointstate
    from massivedatans_amd.like import GaussLineSpectra
    from massivedatans_amd.tablemodel import BROADEN_CUT, TableModel
    lib = _lib.require_device()
    ndata, B, nlive, nx, calls, SETS = (500, 32, 20, 200, 8, 4) if small else (10000, 256, 100, 200, 64, 32)
    plain = big_model([6, 6, 4] if small else [20, 20, 10], 500 if small else 2000, seed=5)
    g = plain.grid
    ext = -0.4 * (3.1 * (g[0] / g) ** 1.3 - 0.8)
    with_e = TableModel(plain.axes, g, plain.table, redshift=True, amplitude=True, extinction=ext)
    with_es = TableModel(plain.axes, g, plain.table, redshift=True, amplitude=True, extinction=ext, broadening=True)
    mid = len(g) // 2
    step = (g[-1] - g[0]) / (len(g) - 1) / g[mid]                          # the mean spacing, relative, at the middle of the grid
    x = np.linspace(g[0] * 1.5, g[-1], nx)
    rng = np.random.RandomState(2)
    truth = params_of(plain, rng, ndata, 1.0)
    y = np.ascontiguousarray(plain.statement(x, truth).T + 0.05 * rng.normal(size=(nx, ndata)))
    spectra = GaussLineSpectra(x, y, noise_level=0.05)
    live = params_of(plain, rng, nlive, 1.0)

    def widen(xs, E, s):
        """(p, z, A) rows as (p, z [, E] [, s], A) rows"""
        cols = [xs[:, :-1]] + ([np.full((len(xs), 1), E)] if E is not None else []) + ([np.full((len(xs), 1), s)] if s is not None else [])
        return np.ascontiguousarray(np.hstack(cols + [xs[:, -1:]]))
    routes = {"plain": (plain, None, None), "E": (with_e, 0.3, None), "Es8": (with_es, 0.3, 8 * step / BROADEN_CUT),
              "Es64": (with_es, 0.3, 64 * step / BROADEN_CUT)}
    tables = {id(m): m.bind(x) for m, _, _ in routes.values()}
    many = params_of(plain, np.random.RandomState(1), SETS * B, 1.0)
    bad = params_of(plain, rng, B, 50.0)                                   # fifty times too bright: nobody takes them
    d_o = lib.mdns_dev_alloc(B * nx * 8)
    ev = (lib.mdns_event_create(), lib.mdns_event_create())
    state, windows = {}, {}
    for name, (tm, E, s) in routes.items():
        xs = widen(many, E, s)
        d_p = lib.mdns_dev_alloc(xs.nbytes)
        _lib.check(lib.mdns_h2d(d_p, _lib.ptr(xs), xs.nbytes), "h2d")
        js = jointstate.CurveJointState(spectra, nlive, None, table=tables[id(tm)])
        js.init(widen(live, E, s))
        js.prepare()
        state[name] = (tm, tables[id(tm)], d_p, js, widen(bad, E, s))
        if s is not None:
            inside = np.abs((g[None, :] - g[:, None]) / g[:, None] / s) <= BROADEN_CUT
            windows[name] = {"knots_at_middle": int(inside[mid].sum()), "knots_longest": int(inside.sum(axis=1).max())}
        if name != "plain":
            fn = lambda xs, _tm=tm: _tm.statement(x, xs)
            js2 = jointstate.CurveJointState(spectra, nlive, fn, ndim=tm.ndim)
            js2.init(widen(live, E, s))
            js2.prepare()
            state["numpy_" + name] = (tm, None, None, js2, widen(bad, E, s))
    kernel_us, chunk_us = {n: [] for n in routes}, {n: [] for n in state}
    # the Python routes first, then the device routes one after the other behind an untimed chunk: a device route
    # timed right after seconds of numpy would be timed on a GPU that had gone idle
    order = sorted(state, key=lambda name: not name.startswith("numpy_"))
    for r in range(rounds + 2):                                            # (two warm-up rounds)
        for name in order:
            tm, table, d_p, js, xs_bad = state[name]
            if name == "plain":
                js.draw_params(xs_bad, None)
            if table is not None:
                _lib.check(lib.mdns_event_record(ev[0]), "event")
                for i in range(calls):
                    _lib.check(lib.mdns_table_curves_batch_dev(table.handle, d_p + (i % SETS) * B * tm.ndim * 8, B, d_o, nx),
                               "mdns_table_curves_batch_dev")
                _lib.check(lib.mdns_event_record(ev[1]), "event")
                t = lib.mdns_event_elapsed_ms(ev[0], ev[1]) * 1e3 / calls
                if r >= 2:
                    kernel_us[name].append(t)
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):
                idx = js.draw_params(xs_bad, None)[0]
            t = (time.perf_counter() - t0) * 1e6
            assert idx == -1
            if r >= 2:
                chunk_us[name].append(t)
    return {"shape": "%d x %d x %d, %d grid knots" % (B, ndata, nx, len(g)), "windows": windows, "kernel_us": kernel_us, "chunk_us": chunk_us}


CHILDREN = {"kernel": (child_kernel, 10), "chunk": (child_chunk, 15), "run": (child_run, 2), "los": (child_los, 5)}


# ------------------------------------------------------------------------------------------ the parent ---------
def main():
    import numpy as np
    small = "--small" in sys.argv
    if "--child" in sys.argv:
        part = sys.argv[sys.argv.index("--child") + 1]
        fn, rounds = CHILDREN[part]
        print(json.dumps(fn(small, 2 if small else rounds)))
        return
    processes = int(sys.argv[sys.argv.index("--processes") + 1]) if "--processes" in sys.argv else 3
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    parts = [a for a in sys.argv[1:] if a in CHILDREN] or list(CHILDREN)
    lines = []
    for part in parts:
        got = []
        for _ in range(processes):                                         # fresh processes
            cmd = [sys.executable, os.path.abspath(__file__), "--child", part] + (["--small"] if small else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                sys.exit("table_bench: part %s failed:\n%s" % (part, (res.stdout + res.stderr)[-3000:]))
            got.append(json.loads(res.stdout.strip().splitlines()[-1]))
        line = {"tool": "table_bench", "part": part, "processes": processes, "small": small}
        if part == "kernel":
            for name in got[0]:
                us = sum((g[name]["us"] for g in got), [])
                med = float(np.median(us))
                rate = got[0][name]["bytes"] / (med * 1e-6)
                line[name] = {"table_MB": got[0][name]["table_MB"], "bytes_per_call": got[0][name]["bytes"], "us_per_call": spread(us),
                              "rate_TBps": round(rate / 1e12, 3), "share_of_gather_rate": round(rate / GATHER_RATE[name], 3)}
        elif part == "chunk":
            line["shape"] = got[0]["shape"]
            for name in got[0]["us"]:
                line[name + "_us"] = spread(sum((g["us"][name] for g in got), []))
            for other in ("numpy", "torch"):
                line["table_vs_" + other] = round(line[other + "_us"]["median"] / line["table_us"]["median"], 2)
        elif part == "los":
            line["shape"], line["windows"] = got[0]["shape"], got[0]["windows"]
            for kind in ("kernel_us", "chunk_us"):
                line[kind] = {name: spread(sum((g[kind][name] for g in got), [])) for name in got[0][kind]}
        else:
            line["shape"], line["ndraws"] = got[0]["shape"], got[0]["ndraws"]
            for name in got[0]["ms"]:
                line[name + "_ms"] = spread(sum((g["ms"][name] for g in got), []))
            line["table_vs_numpy"] = round(line["numpy_ms"]["median"] / line["table_ms"]["median"], 2)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if out_path:
        with open(out_path, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
