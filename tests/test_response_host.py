"""The instrument response on the CPU tier (massivedatans_amd/response.py): ``Response.statement`` against the
sequential statement of include/mdns.h Part 13 and, within the derived bound, against a dense product; the converters
from a dense matrix and from the arrays of an OGIP RMF; every validation rule; and ``problem.CurveProblem(...,
response=)`` over a numpy backend against the response folded into the model by hand."""
import numpy as np
import pytest

from massivedatans_amd import gen, jointstate, problem, sample
from massivedatans_amd.response import Response
from massivedatans_amd.tablemodel import TableModel
from curves_support import NumpyFixedNoise, gauss_prior, line_model
from oracle_backend import patch_neighbors
from response_support import dense_bound, from_rows, lsf_response, random_response, sequential, stress_response
from table_support import same_bits


@pytest.mark.parametrize("nx,n_in,B", [(1, 1, 1), (5, 2, 3), (65, 30, 4), (130, 19, 2), (70, 300, 2)])
def test_statement_equals_the_sequential_loop(nx, n_in, B):
    rng = np.random.RandomState(nx + n_in)
    resp, planted = stress_response(rng, nx, n_in)
    curves = rng.normal(size=(B, n_in))
    curves[0, rng.randint(n_in)] = -0.0
    got = resp.statement(curves)
    assert got.shape == (B, nx) and same_bits(got, sequential(resp, curves))
    # an empty row is +0.0, not -0.0
    empty = np.diff(resp.rowptr) == 0
    assert not np.signbit(got[:, empty]).any() and (got[:, empty] == 0).all()
    assert same_bits(resp.statement(curves[0]), got[0])                   # one curve: [n_in] -> [nx]
    if nx >= 130:
        assert {"empty group", "full row", "one entry", "empty first", "empty last", "negative"} <= set(planted)
    # non-finite bins: the sequential loop's bits, and only the channels whose rows hold the bin
    if n_in > 1:
        bad = curves.copy()
        bad[0, 0], bad[B - 1, n_in - 1] = np.nan, np.inf
        with np.errstate(all="ignore"):
            assert same_bits(resp.statement(bad), sequential(resp, bad))


def test_statement_within_the_bound_of_a_dense_product():
    """On random signed matrices with rows of 0 to 40 entries; the worst share of the bound is printed (DESIGN section 4
    records it)."""
    worst = 0.0
    for seed, (nx, n_in, B) in enumerate([(40, 60, 8), (130, 300, 5), (64, 41, 16), (257, 1100, 3)]):
        rng = np.random.RandomState(seed)
        resp = random_response(rng, nx, n_in, most=40)
        curves = rng.normal(size=(B, n_in)) * 10 ** rng.uniform(-3, 3, size=(B, 1))
        diff = np.abs(resp.statement(curves) - curves @ resp.dense().T)
        bound = dense_bound(resp, curves)
        assert (diff <= bound).all(), (nx, n_in, float((diff / np.where(bound > 0, bound, 1)).max()))
        worst = max(worst, float((diff[bound > 0] / bound[bound > 0]).max()))
    print("worst share of the bound against the dense product: %.3f" % worst)
    assert worst > 0                                                       # (the comparison saw rounding at all)


def test_from_dense_reproduces_the_matrix():
    rng = np.random.RandomState(3)
    R = rng.normal(size=(70, 45)) * (rng.uniform(size=(70, 45)) < 0.2)
    R[0] = 0.0
    R[69] = 0.0
    R[5] = rng.normal(size=45)
    x_in = np.linspace(1.0, 2.0, 45)
    resp = Response.from_dense(R, x_in=x_in)
    assert (resp.nx, resp.n_in, resp.nnz) == (70, 45, int((R != 0).sum())) and resp.x_in is not None
    assert np.array_equal(resp.dense(), R) and (resp.vals != 0).all()
    with pytest.raises(ValueError):
        Response.from_dense(np.zeros(5))
    with pytest.raises(ValueError):
        Response.from_dense(R, x_in=x_in[:-1])


@pytest.mark.parametrize("first_channel", [0, 1])
@pytest.mark.parametrize("with_arf", [False, True])
def test_from_ogip_reproduces_a_dense_reconstruction(first_channel, with_arf):
    """Several groups per bin, bins with no group, padded fixed-width columns, ``first_channel`` 0 and 1, an ``arf``."""
    rng = np.random.RandomState(7 + first_channel)
    n_in, n_channels, width = 23, 40, 3
    n_grp = rng.randint(0, width + 1, size=n_in)
    n_grp[[0, 11]] = 0                                                     # bins no channel sees
    n_grp[5] = width
    f_chan = np.zeros((n_in, width), dtype=np.int64)
    n_chan = np.zeros((n_in, width), dtype=np.int64)
    matrix, dense = [], np.zeros((n_channels, n_in))
    arf = rng.uniform(0.5, 3.0, size=n_in) if with_arf else None
    for i in range(n_in):
        cuts = np.sort(rng.choice(np.arange(1, n_channels), size=2 * n_grp[i], replace=False))
        values = []
        for g in range(n_grp[i]):
            lo, hi = cuts[2 * g], cuts[2 * g + 1]
            f_chan[i, g], n_chan[i, g] = lo + first_channel, hi - lo
            block = rng.uniform(0.01, 1.0, size=hi - lo)
            values.append(block)
            dense[lo:hi, i] = block * arf[i] if with_arf else block
        row = np.concatenate(values) if values else np.zeros(0)
        matrix.append(np.concatenate((row, np.zeros(3))))                  # (a fixed-width column: padded behind)
    resp = Response.from_ogip(n_grp, f_chan, n_chan, matrix, n_channels, first_channel=first_channel, arf=arf)
    assert (resp.nx, resp.n_in) == (n_channels, n_in) and np.array_equal(resp.dense(), dense)
    curves = rng.uniform(size=(3, n_in))
    assert same_bits(resp.statement(curves), sequential(Response.from_dense(dense), curves))
    # one group per bin as scalars
    one = Response.from_ogip(np.ones(4, dtype=int), np.array([0, 1, 2, 3]) + first_channel, np.ones(4, dtype=int), np.arange(1.0, 5.0), 4,
                             first_channel=first_channel)
    assert np.array_equal(one.dense(), np.diag(np.arange(1.0, 5.0)))
    with pytest.raises(ValueError, match="outside the 4 channels"):
        Response.from_ogip([1], [[4 + first_channel]], [[1]], [[1.0]], 4, first_channel=first_channel)
    with pytest.raises(ValueError, match="matrix\\[0\\] holds 1 values"):
        Response.from_ogip([1], [[first_channel]], [[2]], [[1.0]], 4, first_channel=first_channel)
    with pytest.raises(ValueError, match="two groups"):
        Response.from_ogip([2], [[first_channel, first_channel + 1]], [[2, 2]], [[1.0, 2.0, 3.0, 4.0]], 4, first_channel=first_channel)


def test_every_rule_raises_and_names_the_array_and_the_index():
    ok = dict(rowptr=[0, 2, 2, 3], cols=[0, 2, 1], vals=[1.0, -2.0, 0.5], n_in=3)
    assert Response(**ok).nnz == 3
    cases = [
        (dict(rowptr=[1, 2, 2, 3]), "rowptr[0] = 1"),
        (dict(rowptr=[0, 2, 1, 3]), "rowptr[2] = 1 < rowptr[1] = 2"),
        (dict(rowptr=[0, 2, 2, 4]), "cols has shape (3,), rowptr[3] = 4"),
        (dict(rowptr=[0]), "rowptr must be"),
        (dict(cols=[0, 3, 1]), "cols[1] = 3 outside [0, 3) (channel 0)"),
        (dict(cols=[0, -1, 1]), "cols[1] = -1 outside [0, 3) (channel 0)"),
        (dict(cols=[2, 0, 1]), "cols[1] = 0 after 2"),
        (dict(cols=[1, 1, 1]), "cols[1] = 1 after 1"),
        (dict(vals=[1.0, np.nan, 0.5]), "vals[1] = nan is not finite (channel 0)"),
        (dict(vals=[1.0, 2.0, np.inf]), "vals[2] = inf is not finite (channel 2)"),
        (dict(vals=[1.0, 2.0]), "vals has shape (2,)"),
        (dict(n_in=0), "n_in=0"),
        (dict(n_in=(1 << 20) + 1), "n_in=1048577"),
        (dict(cols=[0.0, 2.0, 1.0]), "cols must hold integers"),
        (dict(x_in=[1.0, 2.0]), "x_in has shape (2,)"),
    ]
    for change, words in cases:
        with pytest.raises(ValueError) as err:
            Response(**dict(ok, **change))
        assert words in str(err.value), (change, str(err.value))
    # a row's last column against the next row's first is no rule
    assert Response([0, 1, 2], [2, 0], [1.0, 1.0], 3).nnz == 2
    r = Response(**ok)
    with pytest.raises(ValueError):
        r.statement(np.zeros((2, 4)))


def test_problem_refusals():
    d = gen.horns(5)
    x, y = d["x"][:64], np.ascontiguousarray(d["y"][:64])
    scorer = NumpyFixedNoise(y, 0.01)
    resp = lsf_response(64, 90, 1.5)
    with pytest.raises(ValueError, match="folds onto 63 channels"):
        problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, backend=scorer, response=lsf_response(63, 90, 1.5))
    with pytest.raises(ValueError, match="must be a massivedatans_amd.response.Response"):
        problem.CurveProblem(x, y, line_model(x), gauss_prior, 3, backend=scorer, response=resp.dense())
    tm = TableModel([np.array([0.0, 1.0])], np.array([1.0, 2.0, 3.0]), np.ones((2, 3)))
    with pytest.raises(ValueError, match="x_in"):
        problem.CurveProblem(x, y, tm, gauss_prior, 1, backend=scorer, response=resp)
    # a table model over a numpy backend: its statement on the response's bins, folded by the response's statement
    x_in = np.linspace(1.0, 3.0, 90)
    bound = problem.CurveProblem(x, y, tm, gauss_prior, 1, backend=scorer, response=lsf_response(64, 90, 1.5, x_in=x_in))
    xs = np.array([[0.25], [0.75]])
    assert same_bits(bound.model(xs), bound.response.statement(tm.statement(x_in, xs)))


def test_model_file_response(tmp_path):
    good = tmp_path / "good.py"
    good.write_text("import numpy\nfrom massivedatans_amd.response import Response\nndim = 1\nmodel = lambda xs: xs\n"
                    "priortransform_batch = lambda us: us\nresponse = Response.from_dense(numpy.eye(3))\n")
    assert isinstance(sample.load_model(str(good))["response"], Response)
    bad = tmp_path / "bad.py"
    bad.write_text("import numpy\nndim = 1\nmodel = lambda xs: xs\npriortransform_batch = lambda us: us\nresponse = numpy.eye(3)\n")
    with pytest.raises(ValueError, match="`response` is a ndarray"):
        sample.load_model(str(bad))
    plain = tmp_path / "plain.py"
    plain.write_text("ndim = 1\nmodel = lambda xs: xs\npriortransform_batch = lambda us: us\n")
    assert sample.load_model(str(plain))["response"] is None


def test_whole_run_over_a_numpy_backend_equals_the_folded_model(oracle, monkeypatch):
    """``CurveProblem(..., response=R)`` over a numpy backend against a response-less problem whose model is
    ``lambda xs: R.statement(m(xs))``: the same run, byte for byte."""
    patch_neighbors(monkeypatch, oracle)
    n_in, nx = 90, 64
    x_in = np.linspace(400.0, 800.0, n_in)
    x = np.linspace(400.0, 800.0, nx)
    resp = lsf_response(nx, n_in, 1.5, x_in=x_in)
    fine = line_model(x_in)
    rng = np.random.RandomState(4)
    truth = gauss_prior(rng.uniform(0.2, 0.8, size=(12, 3)))
    y = np.ascontiguousarray(resp.statement(fine(truth)).T + 0.01 * rng.normal(size=(nx, 12)))
    calls = []

    def counted(xs):
        calls.append(len(xs))
        return fine(xs)
    runs = []
    for with_response in (True, False):
        if with_response:
            p = problem.CurveProblem(x, y, counted, gauss_prior, 3, noise_level=0.01, backend=NumpyFixedNoise(y, 0.01), response=resp)
        else:
            p = problem.CurveProblem(x, y, lambda xs: resp.statement(fine(xs)), gauss_prior, 3, noise_level=0.01,
                                     backend=NumpyFixedNoise(y, 0.01))
        assert (p.response is resp) == with_response
        sampler = sample.build_sampler(p, nlive_points=20, nsuperset_draws=10, use_graph=False, seed=1, fused=True)
        with np.errstate(all="ignore"):
            results = sample.integrate(sampler, 0.5, 0, 40)
        assert isinstance(sampler.joint, jointstate.HostJointState) and sampler.ndraws > 0
        runs.append((results["logZ"], results["logZerr"], int(sampler.ndraws), np.array(sampler.pointpilex)))
        mask = np.ones(12, dtype=bool)
        runs[-1] += (p.multi_loglikelihood_batch(truth[:4], mask), p.multi_loglikelihood(truth[1], mask))
    assert calls and runs[0][2] == runs[1][2]
    for k in (0, 1, 3, 4, 5):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
