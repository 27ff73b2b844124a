"""What test_chunk_shapes.py relies on, shown without a device: the planted inputs of ``chunk_support.CHUNK_SHAPES`` keep
clear of their thresholds and blur no pair, the list reaches every branch of the two-launch chunk's dispatch, the restated
route rule follows the library's two switches, and the statement of a draw of several chunks is the reference's rule --
checked by hand on small columns, and run through the sequences of the device test on the reference's likelihoods."""
import numpy as np
import pytest

import chunk_support as cs
import filter_support as fs
from test_commit_record import threshold as record_threshold


@pytest.fixture
def no_switches(monkeypatch):
    monkeypatch.delenv("MDNS_CHUNK_PATH", raising=False)
    monkeypatch.delenv("MDNS_CHUNK_GROUPS", raising=False)


def _route(shape, num_cus=256):
    return cs.expected_route(cs.selection_size(shape), shape[3], shape[2], num_cus)


# ---------------------------------------------------------------------------------------
# preconditions of the planted cases
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", cs.OFFSETS)
@pytest.mark.parametrize("shape", cs.CHUNK_SHAPES, ids=fs.shape_id)
def test_planted_inputs_keep_clear_of_their_thresholds(shape, offset):
    """The assertions of test_filter_shapes.py's test of the same name, and: no pair is blurred by the reference's own
    templates, so the device test compares the chain with L_ref at RTOL_L with no allowance."""
    x, y, params, rows, L_ref = cs.reference(shape, offset)
    ndata, _, nx, B = shape
    assert L_ref.shape == (B, ndata) and (rows is None or (np.diff(rows) > 0).all())
    M = ndata if rows is None else len(rows)
    assert M == cs.selection_size(shape)
    thr = fs.ordinary_thresholds(L_ref, rows)              # asserts the clearance and that someone is accepted
    idx, beats = fs.decision(L_ref, thr, rows)
    assert idx >= 0 and beats.any()
    assert fs.decision(L_ref, fs.unbeatable(L_ref), rows)[0] == -1
    assert not cs.blurred_pairs(x, y, params, L_ref).any()


@pytest.mark.parametrize("shape", cs.CHUNK_SHAPES, ids=fs.shape_id)
def test_a_lone_winner_can_be_planted(shape):
    """The spectra rebuilt from ``own_lines`` are those of ``make_inputs``; with candidate c made the own line of the
    strongest-lined selected spectrum d, c is the maximum of column d by far more than RTOL_L -- for c = B - 1 and for
    the first candidate of the last tile --, and the new candidate blurs no pair either."""
    x, y, params, rows, _ = cs.reference(shape)
    A, mu, sig, noise = cs.own_lines(shape)
    assert np.array_equal(noise + A * np.exp(-0.5 * ((mu.reshape(1, -1) - x.reshape(-1, 1)) / sig) ** 2), y)
    B = shape[3]
    assert cs.lone_candidates(B)[0] == B - 1 and cs.lone_candidates(B)[-1] % 4 == 0 and B - 4 <= cs.lone_candidates(B)[-1] < B
    for c in cs.lone_candidates(B):
        d, planted = cs.lone_winner(shape, c, params, rows)
        assert rows is None or d in rows
        assert np.array_equal(np.delete(planted, c, axis=0), np.delete(params, c, axis=0))
        L = fs.reference_loglike(x, y, planted)
        assert cs.strict_margin(L, c, d) > 1e3 * fs.RTOL_L
        assert not cs.blurred_pairs(x, y, planted, L).any()


# ---------------------------------------------------------------------------------------
# the list reaches its branches
# ---------------------------------------------------------------------------------------
def test_the_shapes_reach_every_branch(no_switches):
    routes = {shape: _route(shape) for shape in cs.CHUNK_SHAPES}
    stages = {}
    for shape, route in routes.items():
        if route is not None:
            stages.setdefault(route, set()).add(cs.cols_nx(shape[2]) // 8)
    # every NST, at its last stage count; <16>, <26> and <32> also at their first (<8> begins at one stage: nx = 1)
    assert stages["k_chunk_accept<8>"] >= {1, 8}
    assert stages["k_chunk_accept<16>"] >= {9, 16}
    assert stages["k_chunk_accept<26>"] >= {17, 26}
    assert stages["k_chunk_accept<32>"] >= {27, 32}
    assert set(stages) == {"k_chunk_accept<%d>" % n for n in (8, 16, 26, 32)}
    two_launch = [s for s in cs.CHUNK_SHAPES if routes[s] is not None]
    classic = [s for s in cs.CHUNK_SHAPES if routes[s] is None]
    # the commit switch: M = 128 | 129
    assert {cs.selection_size(s) for s in two_launch} >= {128, 129}
    assert any(cs.selection_size(s) <= 128 for s in two_launch) and any(cs.selection_size(s) > 1000 for s in two_launch)
    # the channel limit: cols_nx 256 | 264
    assert any(cs.cols_nx(s[2]) == 256 for s in two_launch) and any(cs.cols_nx(s[2]) == 264 for s in classic)
    # the workgroup limit of a 256-CU device: 4096 | 4160
    groups = lambda s: -(-cs.selection_size(s) // 64) * -(-s[3] // 4)
    assert any(groups(s) == 4096 for s in two_launch)
    assert any(groups(s) > 4096 and cs.cols_nx(s[2]) <= 256 and cs.selection_size(s) <= 4096 for s in classic)
    # more than 4096 spectra: B = 8 | 9
    assert any(cs.selection_size(s) > 4096 and s[3] == 8 for s in two_launch)
    assert any(cs.selection_size(s) > 4096 and s[3] == 9 and groups(s) <= 4096 and cs.cols_nx(s[2]) <= 256 for s in classic)
    # partial tiles, the last candidate of 1024, and every shape of the halves is one of the list
    assert any(s[3] % 4 for s in two_launch) and any(s[3] % 4 == 0 for s in two_launch) and any(s[3] == 1024 for s in two_launch)
    assert any(cs.selection_size(s) % 64 for s in two_launch) and any(cs.selection_size(s) % 64 == 0 for s in two_launch)
    assert all(s in two_launch for s in cs.HALVES_SHAPES)
    assert len(classic) == 3


def test_nst_follows_the_stage_count(no_switches):
    for nx, nst in ((1, 8), (8, 8), (64, 8), (65, 16), (128, 16), (129, 26), (208, 26), (209, 32), (256, 32)):
        assert cs.expected_route(10, 1, nx, 256) == "k_chunk_accept<%d>" % nst
    assert cs.expected_route(10, 1, 257, 256) is None
    # the workgroup limit scales with the device
    assert cs.expected_route(4096, 256, 7, 256) is not None and cs.expected_route(4096, 256, 7, 255) is None
    assert cs.expected_route(4096, 1024, 7, 1024) is not None
    assert cs.expected_route(4097, 8, 8, 256) is not None and cs.expected_route(4097, 9, 8, 256) is None
    assert cs.expected_route(4096, 9, 8, 256) is not None


def test_the_switches(monkeypatch, no_switches):
    monkeypatch.setenv("MDNS_CHUNK_PATH", "classic")
    assert all(_route(s) is None for s in cs.CHUNK_SHAPES)
    monkeypatch.setenv("MDNS_CHUNK_PATH", "classical")      # (strcmp: only the word itself)
    assert any(_route(s) is not None for s in cs.CHUNK_SHAPES)
    monkeypatch.delenv("MDNS_CHUNK_PATH")
    monkeypatch.setenv("MDNS_CHUNK_GROUPS", "1")
    single = [s for s in cs.CHUNK_SHAPES if _route(s) is not None]
    assert single and all(cs.selection_size(s) <= 64 and s[3] <= 4 for s in single)
    assert all(_route(s) is None for s in cs.CHUNK_SHAPES if (cs.selection_size(s) > 64 or s[3] > 4))
    for text in ("0", "-3", "", "x"):                       # not positive: the device's own limit
        monkeypatch.setenv("MDNS_CHUNK_GROUPS", text)
        assert _route((4096, None, 7, 256)) is not None and _route((4096, None, 7, 257)) is None
    monkeypatch.setenv("MDNS_CHUNK_GROUPS", "5000 groups")  # atoll reads the leading number
    assert _route((4096, None, 7, 257)) is not None


# ---------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------
def test_the_statement_by_hand():
    """Three data sets, three live points; column by column.  The threshold with n points waiting is the (n + 1)-th
    smallest of live + shelf; a NaN is no value; a comparison is strict."""
    nan = np.nan
    live = np.array([[1.0, 5.0, nan],
                     [3.0, 5.0, 2.0],
                     [2.0, 7.0, 9.0]])
    ref = cs.Statement(live)
    ref.prepare()
    assert np.array_equal(ref.higher, [1.0, 5.0, 2.0])
    #           data set 0  1    2
    L = np.array([[1.0, 5.0, 2.0],       # on every threshold: nobody
                  [0.5, 6.0, nan],       # beats data set 1 only
                  [9.0, 9.0, 9.0]])      # would beat all: never looked at
    assert np.array_equal(ref.votes(L, None), [0, 1, 1])
    idx, beats = ref.chunk(L, None)
    assert idx == 1 and np.array_equal(beats, [False, True, False])
    # data set 1: live 5 5 7 + shelf 6, one waiting: the second smallest, the other 5
    assert np.array_equal(ref.higher, [1.0, 5.0, 2.0]) and np.array_equal(ref.sizes(), [0, 1, 0])
    # the same chunk again: 6 > 5 still; two waiting: the third smallest of 5 5 6 6 7
    idx, beats = ref.chunk(L, None)
    assert idx == 1 and np.array_equal(beats, [False, True, False]) and ref.higher[1] == 6.0
    # and again: 6 ties with the threshold now, so the last candidate is the first that beats anything
    idx, beats = ref.chunk(L, None)
    assert idx == 2 and beats.all()
    # 0: 1 2 3 + 9 -> 2;  1: 5 5 6 6 7 9, three waiting: the fourth -> 6;  2: 2 9 + 9 (NaN is no value) -> 9
    assert np.array_equal(ref.higher, [2.0, 6.0, 9.0]) and np.array_equal(ref.sizes(), [1, 3, 1])
    # a selection: only data sets 0 and 2 are asked, beats is over the selection, data set 1 stays
    rows = np.array([0, 2], dtype=np.int32)
    idx, beats = ref.chunk(np.array([[2.0, 100.0, 9.0], [2.5, 100.0, 9.0]]), rows)
    assert idx == 1 and np.array_equal(beats, [True, False])
    assert np.array_equal(ref.higher, [2.5, 6.0, 9.0]) and np.array_equal(ref.sizes(), [2, 3, 1])
    assert ref.chunk(np.array([[2.5, 100.0, 9.0]]), rows) == (-1, None)
    # one real live value: the threshold is always the point taken in last; no real one: +inf, which nothing beats
    ref = cs.Statement(np.array([[nan, nan], [4.0, nan]]))
    ref.prepare()
    assert np.array_equal(ref.higher, [4.0, np.inf])
    assert ref.chunk(np.array([[5.0, 1e300]]), None)[0] == 0 and ref.higher[0] == 5.0
    assert ref.chunk(np.array([[6.0, np.inf]]), None)[0] == 0 and ref.higher[0] == 6.0
    assert np.array_equal(ref.sizes(), [2, 0])
    assert ref.chunk(np.array([[6.0, np.inf]]), None) == (-1, None)
    # prepare drops what does not lie above the minimum
    ref = cs.Statement(np.array([[1.0], [8.0]]))
    ref.prepare()
    ref.chunk(np.array([[3.0]]), None)
    ref.chunk(np.array([[9.0]]), None)
    ref.live[0, 0] = 3.0
    ref.prepare()
    assert np.array_equal(ref.shelf[0], [9.0]) and ref.higher[0] == 8.0


def test_the_statement_is_the_rule_of_the_commit_record():
    rng = np.random.RandomState(3)
    for _ in range(200):
        col = rng.randint(0, 6, size=rng.randint(1, 7)).astype(np.float64)
        col[rng.uniform(size=len(col)) < 0.2] = np.nan
        shelf = rng.randint(0, 6, size=rng.randint(0, 8)).astype(np.float64)
        assert cs.threshold(col, shelf) == record_threshold(col, shelf)
    bits = rng.uniform(size=131) < 0.5
    words = cs.pack_bits(bits)
    assert len(words) == 3 and all(bool(int(words[k // 64]) >> (k % 64) & 1) == bits[k] for k in range(131))
    assert not int(words[2]) >> 3


def test_check_outcome_wants_the_chain_bits():
    """``check_outcome`` on a made-up chunk: the right outcome passes; a wrong index, a wrong bit, a threshold that is
    the reference's value and not the chain's, and a touched data set outside the selection each fail."""
    L = np.array([[1.0, 1.0, 1.0, 1.0], [3.0, 1.0, 3.0, 3.0]]).astype(np.longdouble)
    Lall = L.astype(np.float64) * (1 + 2.0 ** -50)
    thr = np.array([2.0, 2.0, 0.0, 2.0])
    rows = np.array([0, 1, 3], dtype=np.int32)
    good = (1, np.array([True, False, True]), np.array([Lall[1, 0], 2.0, 0.0, Lall[1, 3]]), np.array([1, 0, 0, 1]))
    cs.check_outcome(good, thr, rows, L, Lall)
    for wrong in ((0,) + good[1:], (1, np.array([True, True, True])) + good[2:],
                  good[:2] + (np.array([3.0, 2.0, 0.0, 3.0]), good[3]),
                  good[:2] + (np.array([Lall[1, 0], 2.0, Lall[1, 2], Lall[1, 3]]), good[3]),
                  good[:3] + (np.array([1, 0, 1, 1]),)):
        with pytest.raises(AssertionError):
            cs.check_outcome(wrong, thr, rows, L, Lall)
    cs.check_outcome((-1, None, thr.copy(), np.zeros(4, dtype=int)), thr, rows, L - 2, Lall - 2)


# ---------------------------------------------------------------------------------------
# what the device test asserts can happen
# ---------------------------------------------------------------------------------------
def _host(live, shelf_cap):
    return None


def test_the_sequences_on_the_reference(no_switches):
    """The three sequences of several chunks with no device, on the reference's likelihoods: the events the device test
    asserts -- repeats that tie, a shelf past the capacity inside one draw, an accepted candidate in every chunk of the
    route switch and of the commit switch -- occur, and the routes are the intended ones."""
    x, y = fs.make_inputs(cs.SEQUENCE_A_SHAPE)[:2]
    log = cs.sequence_a(cs.reference_scorer(x, y), _host, 256)
    assert [B for B, _, _ in log[:5]] == [1, 3, 5, 9, 9] and len(log) >= 11
    assert all(route == "k_chunk_accept<26>" for _, route, _ in log)
    assert len(set(idx for _, _, idx in log)) > 1
    x, y, rows = cs.sequence_b_inputs()
    log = cs.sequence_b(cs.reference_scorer(x, y), _host, 256)
    assert [(B, route) for B, route, _ in log] == [(8, "k_chunk_accept<8>"), (9, None), (4, "k_chunk_accept<8>"),
                                                   (9, None), (8, "k_chunk_accept<8>"), (9, None)]
    x, y = fs.make_inputs((cs.SEQUENCE_C_NDATA, None, cs.SEQUENCE_C_NX, 16))[:2]
    log = cs.sequence_c(cs.reference_scorer(x, y), _host, 256)
    assert [M for M, _, _, _ in log] == [128, 128, 129, 129, 64, 64] and all(route == "k_chunk_accept<8>" for _, _, route, _ in log)


@pytest.mark.parametrize("shape", cs.HALVES_SHAPES, ids=fs.shape_id)
def test_the_halves_have_what_they_need(shape):
    """Under the ordinary thresholds at least two candidates have votes, behind the commit of the second one some
    candidate has none (the foreign vote), and the honest commit takes somebody in: no threshold needs lowering."""
    x, y, params, rows, L_ref = cs.reference(shape)
    thr = fs.ordinary_thresholds(L_ref, rows)
    ref, steps = cs.halves_plan(shape, L_ref.astype(np.float64), thr, rows)
    assert len(steps) == 3
    votes, cleared, second, beats = steps[0]
    assert votes.sum() >= 2 and cleared.sum() == votes.sum() - 1 and beats.any()
    assert steps[1][1].sum() == 1 and not steps[1][0][steps[1][2]] and not steps[1][3].any()
    assert steps[2][2] >= 0 and steps[2][3].any()
    assert ref.sizes().max() == 2 or ref.sizes().max() == 1
