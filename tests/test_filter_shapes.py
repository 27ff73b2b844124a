"""The guarded accept filters (k_gauss_cols_filter; k_gauss_gemm_filter, k_gauss_mfma_filter, k_gauss_mfma_direct
with k_exact_list behind them) at ragged shapes, on selections, at channel counts other than 200 and past the 256
channels the exact re-score holds -- against a plain numpy statement in np.longdouble.

The library reads MDNS_K1_FILTER* once per process, so every mode runs the cases of filter_cases.py in ONE child
pytest process, one after the other, never again; a child that dies by signal, abort or time limit fails its test
and keeps the later ones from starting anything on the GPU.  The thresholds the cases plant come from
filter_support.ordinary_thresholds, whose precondition -- no reference likelihood within 1e-9 of its threshold -- is
checked here without a GPU."""
import os

import numpy as np
import pytest

import filter_support as fs

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "filter_cases.py")


@pytest.fixture(scope="session")
def reference_cache(tmp_path_factory):
    """Where the children keep the np.longdouble references: the first one computes them, the others read them."""
    return tmp_path_factory.mktemp("filter_references")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(fs.MODES))
def test_filter_decides_like_the_plain_statement(mode, reference_cache):
    """Parts A, B and C of filter_cases.py under one filter mode: planted decisions over filter_support.SHAPES,
    the whole joint state against its numpy statement, and the list of the exact re-score overflowing."""
    out = fs.run_child(mode, CASES, cache=reference_cache)
    print(out[-3000:])
    assert "%d passed" % (len(fs.SHAPES) + 9 + 1) in out, out[-3000:]


@pytest.mark.parametrize("shape", fs.SHAPES, ids=fs.shape_id)
def test_planted_inputs_keep_clear_of_their_thresholds(shape):
    """The input builder of the GPU cases on the CPU: for plain and offset data, some candidate is accepted under
    the ordinary thresholds and no reference likelihood of the selection lies within 1e-9 (relative) of its
    threshold (asserted inside ordinary_thresholds), and nobody beats the base thresholds."""
    ndata, sel, nx, B = shape
    for offset in (0.0, 3.0):
        x, y, params, rows, L_ref = fs.reference(shape, offset)
        assert L_ref.dtype == np.longdouble and L_ref.shape == (B, ndata) and y.shape == (nx, ndata)
        if rows is not None:
            assert (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < ndata
            if sel == "1/10":
                assert len(rows) * 8 < ndata and rows[0] > 0 and rows[-1] == ndata - 1
        thr = fs.ordinary_thresholds(L_ref, rows)
        idx, beats = fs.decision(L_ref, thr, rows)
        assert idx >= 0 and beats.any()
        assert fs.decision(L_ref, fs.unbeatable(L_ref), rows)[0] == -1


def test_reference_is_the_sum_it_states():
    """``reference_loglike`` against the sum written out channel by channel with Python's exact rationals."""
    from fractions import Fraction
    x, y, params, _ = fs.make_inputs((3, None, 5, 2))
    L = fs.reference_loglike(x, y, params)
    m = fs.templates(x, params)
    for b in range(2):
        for d in range(3):
            want = Fraction(-1, 2) / Fraction(fs.NOISE) ** 2 * sum((Fraction(m[b, j]) - Fraction(y[j, d])) ** 2 for j in range(5))
            assert abs(Fraction(float(L[b, d])) - want) <= abs(want) * Fraction(1, 10 ** 14)
