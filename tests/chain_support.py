"""Test helpers shared by the tests of the chained first batch (test_pow10.py, test_orchestration.py,
test_muse.py, test_chain.py) and test_joint.py: the lane-kernel scorer, ``pow10_dd`` of
csrc/mdns_pow10.h as a numpy function, and the ctypes request of ``chain_begin``."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LaneScorer(object):
    """``loglike_batch`` that always runs the lane kernel (B >= 32 forces it)."""

    def __init__(self, spectra):
        self.spectra, self.ndata = spectra, spectra.ndata

    def loglike_batch(self, params, data_mask=None):
        params = np.atleast_2d(params)
        B = len(params)
        if B < 32:
            params = np.vstack([params] + [params[-1:]] * (32 - B))
        return self.spectra.loglike_batch(params, data_mask)[:B]


def build_pow10(directory):
    """tests/native/pow10_check.cpp as a shared object in ``directory``: the HOST build of the header the
    chain kernel includes, without contraction like every host file of the product.  Returns
    ``f(v: array) -> array``."""
    so = os.path.join(str(directory), "libpow10_check.so")
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "massivedatans_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "pow10_check.cpp"), "-o", so, "-lm"]
    subprocess.run(cmd, check=True, timeout=300)
    lib = C.CDLL(so)
    lib.pow10_dd_array.restype = None
    lib.pow10_dd_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

    def pow10_dd(v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.empty_like(v)
        if v.size:
            lib.pow10_dd_array(v.ctypes.data, int(v.size), out.ctypes.data)
        return out
    pow10_dd._keep = lib
    return pow10_dd


@pytest.fixture(scope="session")
def pow10_dd(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return build_pow10(tmp_path_factory.mktemp("pow10"))


def make_request(u, mn, mx, prior, limit, mean=None, scale=None):
    """A ``constrainer.ChainRequest`` over numpy arrays (kept alive on the returned object)."""
    from massivedatans_amd import constrainer
    u = np.ascontiguousarray(u, dtype=np.float64)
    keep = [u, np.ascontiguousarray(mn, dtype=np.float64), np.ascontiguousarray(mx, dtype=np.float64)]
    rq = constrainer.ChainRequest()
    rq.n, rq.ndim = u.shape
    dp = C.POINTER(C.c_double)
    rq.u, rq.mn, rq.mx = (a.ctypes.data_as(dp) for a in keep)
    rq.identity = 1 if scale is None else 0
    if scale is not None:
        keep += [np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64)]
        rq.mean, rq.scale = keep[3].ctypes.data_as(dp), keep[4].ctypes.data_as(dp)
    rq.prior = C.pointer(prior)
    rq.limit = int(limit)
    rq._keep = (keep, prior)
    return rq
