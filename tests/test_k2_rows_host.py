"""What tests/test_k2_rows.py leans on, checked without a device: the statement of k2_rows_support against the C oracle
and against itself in float64, and the launch rule's names at the block edges."""
import numpy as np
import pytest

import k2_rows_support as ks


@pytest.mark.parametrize("nx,ndata", [(3, 3), (7, 70), (513, 3), (1537, 5)])
def test_statement_against_the_oracle_and_in_float64(oracle, nx, ndata):
    d = ks.case(nx, ndata, 3)
    want = ks.statement(d["y"], d["v"], d["ypred"])
    assert want.dtype == np.longdouble and want.shape == (3, ndata) and np.all(want < 0)
    mask = np.ones(ndata, dtype=np.bool_)
    for b in range(3):
        got = oracle.muse_like(np.ascontiguousarray(d["y"]), np.ascontiguousarray(d["v"]), np.ascontiguousarray(d["ypred"][b]), mask)
        assert ks.rel_err(got, want[b]) < 1e-12
    own = ks.rel_err(ks.statement(d["y"], d["v"], d["ypred"], dtype=np.float64), want)
    assert own < (1e-13 if nx == 3 else 1e-14), own
    rows = np.array([ndata - 1, 0, ndata - 1])
    assert ks.rel_err(ks.statement(d["y"], d["v"], d["ypred"], rows), want[:, rows]) < 1e-17       # (numpy's sums follow the layout)


def test_the_launch_rule():
    cus = 256
    assert [ks.channel_blocks(nx) for nx in (1, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049, 2560, 2561, 3072, 3073, 3584, 3585, 4096)] == \
        [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8]
    assert ks.expected_kernel(1100, 1, 70, cus) == "k_muse_rows<3, 1>"
    assert ks.expected_kernel(1100, 33, 3, cus) == "k_muse_rows<3, 2>"
    assert ks.expected_kernel(3000, 4, 2 * cus, cus) == "k_muse_rows2<6>"
    assert ks.expected_kernel(3000, 3, 2 * cus, cus) == ks.expected_kernel(3000, 4, 2 * cus - 1, cus) == "k_muse_rows<6, 2>"
    assert ks.expected_kernel(4097, 5, 2 * cus + 1, cus) == ks.expected_kernel(4610, 1, 1, cus) == "k_muse_rows_generic"
    rng = np.random.RandomState(0)
    for ndata in (1, 2, 3, 70):
        ids = ks.scrambled(ndata, rng)
        assert ids.dtype == np.int32 and len(ids) == ndata and ids.max() == ndata - 1 and ids.min() >= 0
        assert ndata < 3 or len(set(ids.tolist())) < ndata
