"""Posterior summaries (mdns.h Part 7) on the CPU tier: no silent fall-back without a device, the header's
declarations, the planning of the .cols parts of a sharded run, and the self-checks of what the GPU tests compare
with (posterior_support.py): the longdouble statement, its derived bounds, the quantile classes and the draws."""
import fractions
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib
from massivedatans_amd.postprocess import plan_parts
import posterior_support as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART7 = ("mdns_posterior_create", "mdns_posterior_destroy", "mdns_posterior_summary", "mdns_posterior_resample",
         "mdns_posterior_timings")


def _no_gpu():
    lib = _lib.load()
    if lib.mdns_device_count() > 0:
        pytest.skip("a GPU is visible")


def test_header_declares_part7():
    with open(os.path.join(ROOT, "include", "mdns.h")) as f:
        text = f.read()
    assert "Part 7" in text
    for name in PART7:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.ABI_SYMBOLS, name
        assert hasattr(_lib.load(), name), name


def test_posterior_without_device_raises():
    _no_gpu()
    from massivedatans_amd.posterior import Posterior
    w = np.zeros((4, 2))
    with pytest.raises(_lib.MdnsError):
        Posterior(w, w, np.zeros((4, 2, 3)))


def test_cli_without_device_fails(tmp_path):
    _no_gpu()
    path = str(tmp_path / "run.npz")
    np.savez(path, logZ=np.zeros(2), logZerr=np.zeros(2), w=np.zeros((4, 2)), L=np.zeros((4, 2)),
             x=np.zeros((4, 2, 3)), u=np.zeros((4, 2, 3)), mask=np.ones((4, 2), bool))
    out = subprocess.run([sys.executable, "-m", "massivedatans_amd.postprocess", path], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
    assert "no HIP device" in out.stderr, out.stderr
    assert not os.path.exists(str(tmp_path / "run.posterior.npz"))


def test_plan_parts_orders_columns():
    groups = plan_parts(["r.cols50-100.npz", "r.cols0-50.npz", "r.cols100-120.hdf5"])
    assert groups == [("r", [("r.cols0-50.npz", 0, 50), ("r.cols50-100.npz", 50, 100), ("r.cols100-120.hdf5", 100, 120)])]


def test_plan_parts_whole_files():
    assert plan_parts(["a.npz", "b.hdf5"]) == [("a", [("a.npz", None, None)]), ("b", [("b.hdf5", None, None)])]
    # two runs' parts side by side: one group each
    g = plan_parts(["a.cols0-2.npz", "b.cols3-4.npz", "a.cols2-5.npz"])
    assert g == [("a", [("a.cols0-2.npz", 0, 2), ("a.cols2-5.npz", 2, 5)]), ("b", [("b.cols3-4.npz", 3, 4)])]


def test_plan_parts_refuses_gap():
    with pytest.raises(ValueError, match="gap"):
        plan_parts(["r.cols0-50.npz", "r.cols60-100.npz"])


def test_plan_parts_refuses_overlap():
    with pytest.raises(ValueError, match="overlap"):
        plan_parts(["r.cols0-50.npz", "r.cols40-100.npz"])
    with pytest.raises(ValueError, match="overlap"):
        plan_parts(["r.cols0-50.npz", "r.cols0-50.hdf5"])


def test_plan_parts_refuses_whole_and_parts():
    with pytest.raises(ValueError):
        plan_parts(["r.npz", "r.cols0-50.npz"])
    with pytest.raises(ValueError):
        plan_parts(["r.cols5-5.npz"])


def test_cli_refuses_gap_before_touching_the_device(tmp_path):
    out = subprocess.run([sys.executable, "-m", "massivedatans_amd.postprocess", "r.cols0-5.npz", "r.cols6-9.npz"],
                         cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0 and "gap" in out.stderr


def test_run_outputs_untouched_without_switch(tmp_path, monkeypatch):
    from massivedatans_amd.postprocess import run_posterior_outputs
    monkeypatch.delenv("MDNS_POSTERIOR", raising=False)
    assert run_posterior_outputs(str(tmp_path / "run"), dict(weights=[])) is None
    assert os.listdir(str(tmp_path)) == []


# ---- the statement, the bounds and the inputs of the GPU tests (posterior_support.py), without a device ---------

ALL_CASES = ps.all_cases()
_IDS = [c[0] for c in ALL_CASES]


@pytest.mark.parametrize("n,nsamp", [(1, 1), (1, 5), (2, 2), (4, 7), (8, 8), (16, 21)])
def test_statement_against_fractions(n, nsamp):
    """Equal lw on n = 2^k rows: p = 1 / n, and every output is a rational number (log_norm - lw = log n aside)."""
    Fr = fractions.Fraction
    rng = np.random.default_rng(n + nsamp)
    w = np.full((nsamp, 1), -np.inf)
    rows = np.sort(rng.choice(nsamp, n, replace=False))
    w[rows, 0] = 0.0
    L = np.full((nsamp, 1), -1.75)
    x = np.round(rng.normal(size=(nsamp, 1, 2)) * 8) / 4                 # short dyadic values, with ties
    q = np.array([1e-300, 0.25, 0.5, 0.5 + 2.0 ** -40, np.nextafter(0.25, 1), 0.75, 1.0])
    st = ps.statement(w, L, x, q)
    assert st['nfinite'][0] == n and st['imaxL'][0] == rows[0]
    assert st['ess'][0] == n and st['tbar'][0] == 0
    assert abs(st['log_norm'][0] - (ps.LD(-1.75) + np.log(ps.LD(n)))) <= 2.0 ** -62
    for k in range(2):
        v = [Fr(float(t)) for t in x[rows, 0, k]]
        mean = sum(v) / n
        var = sum((t - mean) ** 2 for t in v) / n
        # longdouble carries 64 bits: sums of at most 16 terms of order 1 and a square root stay within 2^-60 and
        # 2^-58 of the rational value (relative to a scale of at least 1 and 2^-20)
        assert abs(st['mean'][0, k] - ps.LD(mean.numerator) / ps.LD(mean.denominator)) <= 2.0 ** -60
        want = np.sqrt(ps.LD(var.numerator) / ps.LD(var.denominator))
        assert abs(st['std'][0, k] - want) <= 2.0 ** -58 * max(float(want), 2.0 ** -20)
        assert abs(st['A'][0, k] - float(sum(abs(t) for t in v) / n)) <= 2.0 ** -50
        for j, qq in enumerate(q):
            first = min(t for t in v if Fr(sum(1 for s in v if s <= t), n) >= Fr(float(qq)))
            assert st['qclass'][0, k, j] == ps.EXACT
            assert Fr(float(st['quant'][0, k, j])) == first, (k, j)


@pytest.mark.parametrize("case", ALL_CASES, ids=_IDS)
def test_emulation_within_bounds(case):
    """numpy float64 in the kernels' own order lies within every derived bound of the longdouble statement, and
    its integer select returns the statement's value wherever that is determined."""
    w, L, x, q, st = ps.stated(case)
    ps.check_against_statement(ps.emulate(w, L, x, q), st, seen=dict(log_norm=0.0, ess=0.0, mean=0.0, std=0.0))


@pytest.mark.parametrize("case", ALL_CASES, ids=_IDS)
def test_no_slivers(case):
    """Every quantile of every input is determined: class must, or exact in the built ties (and only there)."""
    st = ps.stated(case)[4]
    ok = st['nfinite'] > 0
    assert not np.any(st['qclass'][ok] == ps.SLIVER), np.argwhere(st['qclass'] == ps.SLIVER)[:5]
    if case[0].startswith("ties-"):
        assert np.all(st['qclass'] == ps.EXACT)
    elif case[0].startswith(("keys-", "silent-")):                       # elsewhere a column of one finite row is dyadic too
        assert np.all(st['qclass'][ok] == ps.MUST)


def test_ties_are_ties():
    """The dyadic inputs put the target on a cumulative weight exactly, and the neighbours of q move the answer."""
    for case in ps.quantile_cases():
        if not case[0].startswith("ties-"):
            continue
        w, L, x, q, st = ps.stated(case)
        n = int(case[0].split("-")[2])
        for d in range(w.shape[1]):
            v = np.sort(x[np.isfinite(w[:, d]), d, 0])
            assert len(v) == n
            c = np.arange(1, n + 1) / n
            want = v[np.minimum(np.searchsorted(c, q, 'left'), n - 1)]
            assert np.array_equal(st['quant'][d, 0], want)
        assert n == 1 or len(np.unique(st['quant'][0, 0])) > len(q) // 5


def _resample_runs():
    for nsamp in ps.RESAMPLE_NSAMP:
        yield ps.resample_input(nsamp), ps.resample_calls(nsamp)
    yield ps.resample_input(257), ps.key_calls()
    for nsamp in ps.PLACEMENT_NSAMP:
        yield ps.placement_input(nsamp), [(257, 2 ** 63 + 5, 100), (4001, 0, 2 ** 40)]
    for shape in ps.BATCH_SHAPES:
        yield ps.batch_input(shape), [ps.BATCH_DRAWS]


def test_draws_clear_the_boundaries():
    """No reference draw of any resampling test lies within the clearance of a cdf boundary."""
    total = 0
    for (w, L, x), calls in _resample_runs():
        for n, seed, col in calls:
            for d in range(w.shape[1]):
                idx, near = ps.draws(w, L, d, seed, col, n)
                assert near.min() > ps.clearance(w.shape[0]), (w.shape, n, seed, col, d)
                total += int((idx >= 0).sum())
    assert total > 10000


def test_shapes_straddle_the_constants():
    nsamps = {s[0] for s in ps.SHAPES}
    assert nsamps == set(ps.NSAMP_AXIS) and {s[1] for s in ps.SHAPES} == set(ps.NDATA_AXIS)
    assert {s[2] for s in ps.SHAPES} == set(range(1, ps.K_POST_DIM + 1))
    ragged = {s[2] for s in ps.SHAPES if s[0] % 64 and s[1] % 64 and s[1] > 1}
    assert ragged == set(range(1, ps.K_POST_DIM + 1))
    plans = {n: ps.plan(n) for n in nsamps}
    for at in (ps.K_QLDS, ps.K_SLICE_ROWS, ps.K_QBLOCK, 64 * ps.K_SLICE_ROWS):
        assert {at - 1, at, at + 1} <= nsamps, at
    assert plans[ps.K_QLDS]['staged'] and not plans[ps.K_QLDS + 1]['staged']
    assert plans[128]['nslices'] == 1 and plans[129]['nslices'] == 2
    assert plans[8192]['rows_per_slice'] == 128 and plans[8193]['rows_per_slice'] == 129       # longer slices
    assert plans[8192]['nslices'] == 64 and plans[8193]['nslices'] == 64
    assert plans[255]['chunk'] == plans[256]['chunk'] == 1 and plans[257]['chunk'] == 2
    assert {ps.plan(n)['staged'] for n in ps.QUANTILE_NSAMP} == {True, False}
    assert any(n % 4 == 3 for n in ps.N_AXIS) and {n % 4 for n in ps.N_AXIS} == {1, 2, 3}
    assert max(ps.SEED_AXIS) == 2 ** 64 - 1 and any(2 ** 32 <= s for s in ps.SEED_AXIS)
    assert max(ps.COLUMN_AXIS) >= 2 ** 32
    # the batches: every asked-for size is what post_batch makes of the budget, for both kinds of scratch
    for nsamp, ndata, ndim in ps.BATCH_SHAPES:
        sizes = ps.batch_sizes(ndata)
        assert {1, 64, 65, ndata} <= set(sizes)
        assert any(ndata % b and b < ndata for b in sizes)                   # a final short batch
        for b in sizes:
            for per in (ps.summary_bytes(nsamp, ndim), ps.resample_bytes(nsamp)):
                assert ps.batch_of(b * per, per, ndata) == b == ps.batch_of(b * per + per - 1, per, ndata)
        assert ps.batch_of(ps.K_SCRATCH_BYTES, ps.summary_bytes(nsamp, ndim), ndata) == ndata   # unbatched by default
