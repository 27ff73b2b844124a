"""Posterior summaries (mdns.h Part 7) on the CPU tier: no silent fall-back without a device, the header's
declarations, and the planning of the .cols parts of a sharded run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib
from massivedatans_amd.postprocess import plan_parts

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
