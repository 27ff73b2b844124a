"""The K2 matrix-core filter (csrc/mdns_k2gemm.hip: k_muse_gemm_band_sk<NC, TILED>, k_muse_gemm_band<NC, KW> and the
hand-over of split tiles between workgroups) on its OWN decisions -- the votes, marks and count of
mdns_muse_filter_dev, and mdns_backend_draw_band where the filter settles the chunk -- against a plain statement in
np.longdouble (k2_filter_support.py), at ragged shapes, on selections, with every instantiation and forced numbers
of workgroups.

The library reads MDNS_K2_FILTER_* once per process, so every configuration runs the cases of k2_filter_cases.py in
ONE child pytest process, never again; a child that dies by signal, abort or time limit fails its test and keeps the
later ones from starting anything on the GPU.  What the cases need of their inputs -- no pair in the sliver between two
demands, and every kind of demand present -- is checked here without a GPU."""
import os
from fractions import Fraction

import numpy as np
import pytest

from massivedatans_amd import gen
import k2_filter_support as ks

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k2_filter_cases.py")
#: Part A (one per shape), Part B (three shapes), Part C
NCASES = len(ks.SHAPES) + 3 + 1


@pytest.fixture(scope="session")
def k2_reference_cache(tmp_path_factory):
    """Where the children keep the np.longdouble references: the first one computes them, the others read them."""
    return tmp_path_factory.mktemp("k2_filter_references")


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(ks.CONFIGS))
def test_k2_filter_decides_like_the_plain_statement(config, k2_reference_cache):
    """Parts A, B and C of k2_filter_cases.py under one configuration; each case asserts the kernel instantiation
    that scored it."""
    out = ks.run_child(config, CASES, cache=k2_reference_cache)
    print(out[-3000:])
    assert "%d passed" % NCASES in out, out[-3000:]


@pytest.mark.parametrize("shape", ks.SHAPES, ids=ks.shape_id)
def test_inputs_leave_no_sliver_and_hold_every_class(shape):
    """On the reference alone, over all launches of a shape: no selected pair lies in the sliver between two demands
    (the condition allows 1 %; the seeds give none), some launch has a candidate that must clear, some a pair that
    must be listed, some a candidate that must stay silent; every pair with the NaN spectrum must be listed; and the
    unselected data sets carry the threshold -1e300."""
    case = ks.Case(shape)
    A, Lq = case.reference()
    assert Lq.dtype == np.longdouble and A.dtype == np.longdouble and Lq.shape == (case.B, case.ndata) and np.isfinite(Lq).all()
    if case.rows is not None:
        assert (np.diff(case.rows) > 0).all() and case.rows[0] >= 0 and case.rows[-1] < case.ndata and len(case.rows) == case.M
        if shape[3] == "third":
            assert case.rows[0] == 0 and case.rows[-1] == case.ndata - 1
    plain = gen.muse_like(case.ndata, case.nx)["y"]
    third = np.arange(case.ndata) % 3 == 1
    assert np.array_equal(case.y[:, third], plain[:, third] * 1e3) and np.array_equal(case.y[:, ~third], plain[:, ~third])
    slivers, pairs, clear, listed, silent = ks.preconditions(case)
    assert pairs == 2 * ks.DRAWS * case.B * case.M
    assert slivers == 0, "%d of %d pairs in the sliver: another seed" % (slivers, pairs)
    assert clear > 0 and listed > 0 and silent > 0, (clear, listed, silent)
    k = int(np.flatnonzero(case.sel == case.d_nan)[0])
    unselected = np.setdiff1d(np.arange(case.ndata), case.sel)
    for with_nan, bound, thr in case.launches():
        assert (thr[unselected] == -1e300).all() and (thr[case.sel] > -1e300).all()
        if with_nan:
            assert case.classify(with_nan, bound, thr)["must_list"][:, k].all()
    if shape == ks.SHAPES[ks.REPEAT_SHAPE]:
        assert ks.preconditions(case, draws=ks.REPEATS // 10, first_draw=3)[0] == 0


def test_shapes_reach_every_instantiation():
    """The rule of launch_muse_filter restated in k2_filter_support.expected_kernel names, over the shapes and the
    configurations, all six stream-K instantiations and all six of the whole-tile family."""
    names = set()
    for config in ks.CONFIGS:
        for shape in ks.SHAPES:
            case = ks.Case(shape)
            names.add(ks.expected_kernel(config, case.ndata, case.nx, case.B, case.rows, case.M))
    want = {"k_muse_gemm_band_sk<%d%s>" % (nc, t) for nc in (1, 2, 4) for t in ("", ", tiled")}
    want |= {"k_muse_gemm_band<%d, %d>" % (nc, kw) for nc in (1, 2, 4) for kw in (4, 8)}
    assert names == want, sorted(want ^ names)


def test_statement_is_the_sums_it_states():
    """``reference_filter`` against the same definitions written out channel by channel in exact rationals."""
    case = ks.Case((3, 5, 2, None, 0))
    A, Lq = ks.reference_filter(case.y, case.v, case.templates)
    for d in range(3):
        y = [Fraction(float(t)) for t in case.y[:, d]]
        w = [Fraction(float(1.0 / t)) for t in case.v[:, d]]
        a = sum(yj * yj * wj for yj, wj in zip(y, w))
        assert abs(Fraction(float(A[d])) - a) <= abs(a) * Fraction(1, 10 ** 14)
        for b in range(2):
            m = [Fraction(float(t)) for t in case.templates[b]]
            s = sum(yj * wj * mj for yj, wj, mj in zip(y, w, m)) / (Fraction(1e-10) + sum(wj * mj * mj for wj, mj in zip(w, m)))
            want = Fraction(-1, 2) * sum((yj - s * mj) ** 2 * wj for yj, wj, mj in zip(y, w, m))
            assert abs(Fraction(float(Lq[b, d])) - want) <= abs(want) * Fraction(1, 10 ** 14)
