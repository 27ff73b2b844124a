"""The CPU side of the region kernels' shape tests (tests/test_region_shapes.py): the numpy statement of K3 / K5 / K6
against the C oracle, bit for bit, and the launch rules restated in tests/region_support.py at their edges -- with
every parametrised GPU case asserted to reach the instantiation and geometry it is meant for (256 CUs), so that a later
change of a launch rule that silently moves a case off its edge fails here."""
import numpy as np
import pytest

import region_support as rs

CUS = 256


# ------------------------------------------------------------------------------------------ statement against oracle
def _agree(oracle, pool, chosen):
    pool, chosen = np.ascontiguousarray(pool), np.ascontiguousarray(chosen)
    want = oracle.bootstrapped_maxdistance(pool, chosen)
    assert rs.bootstrap_radius(pool, chosen) == want
    nn = oracle.most_distant_nearest_neighbor(pool)
    assert rs.nn_radius(pool) == nn
    rng = np.random.RandomState(len(pool))
    for r in (want, nn, 0.5 * (want + nn)):
        pts = np.ascontiguousarray(np.vstack((rs.boundary_points(pool, r), pool[rng.randint(0, len(pool), size=9)] + 0.3 * r * rng.normal(size=(9, pool.shape[1])))))
        full = oracle.count_within_distance_of(pool, r, pts, countmax=0)
        assert np.array_equal(rs.count_within(pool, r, pts), full)
        assert np.array_equal(np.minimum(rs.count_within(pool, r, pts), 1), oracle.count_within_distance_of(pool, r, pts, countmax=1))
    return want, nn


@pytest.mark.parametrize("K,ndim,nboot", [(1, 1, 1), (2, 3, 10), (63, 16, 11), (700, 3, 33), (2049, 5, 16)])
def test_statement_against_the_oracle(K, ndim, nboot, oracle):
    pool = rs.hurtful_pool(K, ndim, rs.pool_rng(K, ndim))
    _agree(oracle, pool, rs.draw_choice(K, nboot, rs.pool_rng(K, ndim, nboot)))


@pytest.mark.parametrize("kind", rs.DEGENERATE)
@pytest.mark.parametrize("K,ndim", rs.DEGENERATE_POOLS)
def test_statement_on_degenerate_rounds(K, ndim, kind, oracle):
    pool = rs.hurtful_pool(K, ndim, rs.pool_rng(K, ndim))
    for nboot in (10, 3, 12):
        chosen = rs.degenerate_choice(kind, K, nboot, rs.pool_rng(K, ndim, nboot))
        want, _ = _agree(oracle, pool, chosen)
        if kind == "nobody":
            assert want == (np.sqrt(1e300) if K > 1 else 0.0)
        if kind in ("everybody", "only0_out"):
            assert want == 0.0
        assert np.array_equal(rs.pack(chosen), (chosen * (1 << np.arange(nboot))).sum(axis=1).astype(np.uint32))


def test_statement_on_odd_choice_values(oracle):
    for K, ndim, nboot in ((300, 3, 11), (2049, 9, 17)):
        pool = rs.hurtful_pool(K, ndim, rs.pool_rng(K, ndim))
        odd, plain = rs.odd_choice(K, nboot, rs.pool_rng(K, ndim, 3))
        assert np.isnan(odd).any() and (odd == 5e-324).any() and (odd == 0.5).any() and (odd == -1.0).any()
        assert (np.signbit(odd) & (odd == 0)).any() and (~np.signbit(odd) & (odd == 0)).any()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(odd != 0, plain != 0)
        want, _ = _agree(oracle, pool, odd)
        assert want == oracle.bootstrapped_maxdistance(pool, np.ascontiguousarray(plain)) == rs.bootstrap_radius(pool, plain) > 0


@pytest.mark.parametrize("scale", rs.SCALES)
def test_statement_at_extreme_scales(scale, oracle):
    pool = rs.hurtful_pool(50, 2, rs.pool_rng(50, 2), scale)
    want, nn = _agree(oracle, pool, rs.draw_choice(50, 10, rs.pool_rng(50, 2, 10)))
    if scale == 1e-160:
        assert 0 < want < 1e-159
    if scale == 1e150:
        assert 1e140 < want < 1e150 and nn == 1e150
    if scale == 3e153:
        assert want == 1e150 and nn == 1e150


def test_boundary_points_are_exact():
    """the points differ from a member along one axis only, by r, its neighbours and -r, exactly"""
    pool = rs.hurtful_pool(400, 3, rs.pool_rng(400, 3))
    for r in (0.123456789, 1e150, 3.7e-161):
        pts = rs.boundary_points(pool, r)
        d = rs.sq_distances(pts, pool)
        with np.errstate(over="ignore", under="ignore"):
            exact = [np.float64(x) * np.float64(x) for x in (r, np.nextafter(r, 0.0), np.nextafter(r, np.inf))]
        assert len(pts) > 3 + 8
        for p in range(len(pts) - 3):
            assert any((d[p] == e).any() for e in exact), p
    assert len(rs.boundary_points(pool[:1], 0.0)) >= 1


def test_garbage_bits_stay_below_sixteen():
    rng = np.random.RandomState(3)
    for nboot in rs.GARBAGE_ROUNDS:
        chosen = rs.draw_choice(100, nboot, rng)
        masks = rs.with_garbage(rs.pack(chosen), nboot, rng)
        assert np.array_equal(masks & np.uint32((1 << nboot) - 1), rs.pack(chosen))
        assert (masks >> np.uint32(nboot)).any() and not (masks >> np.uint32(16)).any()


# ------------------------------------------------------------------------------------------ launch rules at their edges
def test_count_rule_at_the_throughput_edge():
    assert rs.sl1_sizes(CUS) == (32705, 32768)
    for ndim, D in ((3, 3), (8, 8), (9, 0)):
        assert rs.count_launch(32704, 70, ndim, False, CUS)[:2] == ("k_count_within<%d, 4>" % D, 16)
        assert rs.count_launch(32705, 70, ndim, False, CUS)[:2] == ("k_count_within<%d, 1>" % D, 64)
        assert rs.count_launch(32704, 70, ndim, True, CUS)[:2] == ("k_count_within<%d, 16>" % D, 4)
        assert rs.count_launch(32705, 70, ndim, True, CUS)[:2] == ("k_count_within<%d, 1>" % D, 64)
    assert rs.count_launch(40000, 400, 3, True, CUS) == ("k_count_within<3, 1>", 64, 512, 1, 512)


def test_count_rule_on_the_ndim_ladder():
    tiles = {14: 512, 15: 496, 16: 464, 32: 224, 100: 64}
    for ndim, tile_n in tiles.items():
        name, pts, got, gy, kchunk = rs.count_launch(30, 2 * tile_n + 1, ndim, False, CUS)
        assert (name, pts, got) == ("k_count_within<0, 4>", 16, tile_n)
        assert gy == 3 and kchunk == tile_n                       # 30 points: two workgroups, split as far as the tiles go
    top = rs.max_ndim("count")
    assert top == 472 and rs.count_launch(30, 33, top, False, CUS)[2:] == (16, 3, 16)
    assert rs.count_launch(30, 33, top + 1, False, CUS) is None and rs.count_launch(30, 33, top + 1, True, CUS) is None
    assert rs.dim_case(8) == 8 and rs.dim_case(9) == 0


def test_count_rule_splits_the_members():
    for (M, K), gy in rs.SPLIT_GY.items():
        name, pts, tile_n, got, kchunk = rs.count_launch(M, K, 3, False, CUS)
        assert (name, pts, tile_n, got, kchunk) == ("k_count_within<3, 4>", 16, 512, gy, 512)
        assert rs.count_launch(M, K, 3, True, CUS)[3] == 1       # a mailbox: no partial counts
    assert K - (gy - 1) * kchunk == 392
    assert 513 - 512 == 1 and 1025 - 2 * 512 == 1               # the last chunk is ONE member
    # rounding of the chunk to a multiple of the tile: 5000 members over 4 chunks of 1250 -> 1536 = 3 tiles, 4 chunks
    assert rs.count_launch(2100, 5000, 3, False, CUS)[3:] == (4, 1536)


def test_radius_rules_at_their_edges():
    for K in rs.sl1_sizes(CUS):
        assert rs.nearest_launch(K, 3, None, False, False, CUS)["windows"] == [("k_nearest_chosen<3, true, 1, 10>", 512)]
        assert rs.nearest_launch(K, 3, 3, False, True, CUS)["windows"] == [("k_nearest_chosen<3, false, 1, 10>", 512)]
        assert rs.nearest_launch(K, 6, 11, True, True, CUS)["windows"] == [("k_nearest_chosen<6, false, 1, 16>", 512)]
        assert rs.nearest_launch(K, 3, 3, True, True, CUS)["windows"][0][0] == "k_nearest_uniform<3, 10>"
        assert rs.nearest_launch(K, 6, 3, True, True, CUS)["windows"] == [("k_nearest_chosen<6, false, 1, 10>", 512)]
    assert rs.nearest_launch(32704, 3, None, False, False, CUS)["windows"] == [("k_nearest_chosen<3, true, 4, 10>", 512)]
    # the uniform path
    want = {640: (5, 128, 128), 641: (5, 132, 144), 2048: (16, 128, 128), 2049: (16, 132, 144), 8193: (16, 516, 512)}
    for K, geometry in want.items():
        assert rs.nearest_launch(K, 3, 10, True, True, CUS)["uniform"] == geometry
    assert rs.nearest_launch(639, 3, 10, True, True, CUS)["uniform"] is None
    assert rs.nearest_launch(640, 6, 10, True, True, CUS)["uniform"] is None
    assert rs.uniform_tiles(8193, 3, 10) == ([512, 4], [453])
    assert rs.uniform_tiles(641, 5, 16) == ([132], [113])
    # tiles shrink from about ndim 14 on, depending on the rounds carried
    assert [rs.nearest_launch(40, n, None, False, False, CUS)["windows"][0][1] for n in (14, 15)] == [512, 480]
    assert [rs.nearest_launch(40, n, 10, True, True, CUS)["windows"][0][1] for n in (13, 14)] == [512, 480]
    assert [rs.nearest_launch(40, n, 11, False, True, CUS)["windows"][0][1] for n in (12, 13)] == [512, 480]
    assert (rs.max_ndim("nearest"), rs.max_ndim("bootstrap", 10), rs.max_ndim("bootstrap", 11)) == (475, 439, 415)
    for kind, nboot in (("nearest", None), ("bootstrap", 10), ("bootstrap", 11)):
        top = rs.max_ndim(kind, nboot)
        assert rs.nearest_launch(40, top, nboot, False, True, CUS)["windows"][0][1] == 16
        assert rs.nearest_launch(40, top + 1, nboot, False, True, CUS) is None


def test_round_windows_of_the_f64_paths():
    names = {n: [w[0][-3:-1] for w in rs.nearest_launch(300, 3, n, False, True, CUS)["windows"]] for n in rs.ROUND_COUNTS}
    assert names == {1: ["10"], 9: ["10"], 10: ["10"], 11: ["16"], 16: ["16"], 17: ["16", "10"], 32: ["16", "16"], 33: ["16", "16", "10"]}
    for nboot in rs.ROUND_COUNTS:
        for K, ndim in rs.F64_POOLS:
            region = rs.nearest_launch(K, ndim, nboot, False, True, CUS)
            dropin = rs.nearest_launch(K, ndim, nboot, False, False, CUS)
            assert region["fused"] == (K <= 2048) and region["packs"] == (K > 2048) and dropin["packs"] and not dropin["fused"]
            assert region["own_rounds"] == (nboot > 16) and not dropin["own_rounds"]
            assert region["windows"] == dropin["windows"] and len(region["windows"]) == (nboot + 15) // 16
            assert all(("<%d, false, 4, " % rs.dim_case(ndim)) in w[0] for w in region["windows"])


# ------------------------------------------------------------------------------------------ the GPU cases reach their edges
def test_the_polled_cases_reach_their_instantiations():
    seen = set()
    for K, ndim in rs.POLLED_SHAPES:
        for M in rs.POLLED_WALK:
            name, pts, tile_n, gy, kchunk = rs.count_launch(M, K, ndim, True, CUS)
            assert gy == 1 and kchunk >= K
            assert (name, pts) == ("k_count_within<%d, %d>" % (rs.dim_case(ndim), 1 if M == 40000 else 16), 64 if M == 40000 else 4)
            seen.add(name)
            seen.add(rs.count_launch(M, K, ndim, False, CUS)[0])
    assert {"k_count_within<0, 16>", "k_count_within<0, 1>", "k_count_within<0, 4>", "k_count_within<3, 16>", "k_count_within<8, 1>"} <= seen
    assert rs.count_launch(5, 300, 16, True, CUS)[2] == 464                     # (300, 16): a shrunken tile
    assert rs.count_launch(5, 1025, 9, True, CUS)[2:] == (512, 1, 1536)          # three tiles, the last of one member
    # M = 3, 4, 5 straddle the 4 points of a fine workgroup; 63 | 257 its 16 waves' worth; 1000 is the sampler's own call
    assert [rs.count_launch(M, 400, 3, True, CUS)[1] for M in (3, 4, 5)] == [4, 4, 4]


def test_the_split_cases_reach_their_splits():
    for M, K, ndim in rs.SPLIT_CASES:
        name, pts, tile_n, gy, kchunk = rs.count_launch(M, K, ndim, False, CUS)
        assert name == "k_count_within<%d, 4>" % rs.dim_case(ndim) and tile_n == 512 and kchunk == 512
        assert gy == rs.SPLIT_GY.get((M, K), 10)


def test_the_ladder_cases_reach_shrunken_tiles():
    last = rs.MAX_TILE + 1
    for step in rs.NDIM_LADDER:
        ndim = rs.ladder_ndim(step, "count")
        tile_n = rs.count_launch(30, 1, ndim, False, CUS)[2]
        assert tile_n < last or step == 14
        last = tile_n
        assert rs.count_launch(30, 2 * tile_n + 1, ndim, True, CUS)[:2] == ("k_count_within<0, 16>", 4)
        for kind, nboot in (("nearest", None), ("bootstrap", 10), ("bootstrap", 11)):
            ndim = rs.ladder_ndim(step, kind, nboot)
            plan = rs.nearest_launch(40, ndim, nboot, nboot == 10, True, CUS)
            t = plan["windows"][0][1]
            assert 16 <= t <= 512 and (t < 512 or step == 14) and t + 1 < rs.UNIFORM_LEAST
            assert plan["windows"][0][0] == "k_nearest_chosen<0, %s, 4, %d>" % ("true" if nboot is None else "false", 16 if nboot == 11 else 10)
    assert last == 16


def test_the_packed_cases_reach_their_kernels():
    for K, ndim in rs.PACKED_LARGE:
        for nboot, rt in ((10, 10), (16, 16), (3, 10)):
            plan = rs.nearest_launch(K, ndim, nboot, True, True, CUS)
            if ndim <= 5:
                assert plan["windows"][0][0] == "k_nearest_uniform<%d, %d>" % (ndim, rt)
                ny, kchunk, tile_n = plan["uniform"]
                assert K % kchunk != 0 and (K - (ny - 1) * kchunk) % 4 != 0      # a ragged last chunk
            else:
                assert plan["windows"] == [("k_nearest_chosen<%d, false, 4, %d>" % (rs.dim_case(ndim), rt), 512)]
    for K, ndim in rs.GARBAGE_POOLS:
        for nboot in rs.GARBAGE_ROUNDS:
            name = rs.nearest_launch(K, ndim, nboot, True, True, CUS)["windows"][0][0]
            rt = 16 if nboot > 10 else 10
            assert name == ("k_nearest_uniform<3, %d>" % rt if (K, ndim) == (700, 3) else "k_nearest_chosen<%d, false, 4, %d>" % (ndim, rt))
    for K, ndim in rs.DEGENERATE_POOLS:
        assert (rs.nearest_launch(K, ndim, 12, True, True, CUS)["uniform"] is not None) == (K == 700)
    # the sequence on one handle: uniform, fused f64 with a round buffer of its own, uniform with 16 rounds, fused 11
    assert rs.nearest_launch(700, 3, 33, False, True, CUS)["own_rounds"] and rs.nearest_launch(700, 3, 33, False, True, CUS)["fused"]
    assert rs.nearest_launch(700, 3, 16, True, True, CUS)["windows"][0][0] == "k_nearest_uniform<3, 16>"
    assert rs.nearest_launch(700, 3, 11, False, True, CUS)["windows"] == [("k_nearest_chosen<3, false, 4, 16>", 512)]
