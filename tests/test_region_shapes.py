"""The RadFriends region kernels (csrc/mdns_neighbors.hip, csrc/mdns_geom.h, the region handles of csrc/mdns_core.hip)
at their tile, slice, chunk and round edges: the membership count (K3/K4), the nearest-neighbour radius (K5) and the
bootstrapped radius (K6) against the plain numpy statement of tests/region_support.py, bit for bit -- every comparison
is ``==`` or ``array_equal``.

Where a case is built for one instantiation the launch is followed by a look at ``mdns_profile_kernel(2)`` (K3) or
``(3)`` (K5/K6): a case that takes another kernel than the one it was built for fails instead of passing vacuously.
tests/test_region_shapes_host.py asserts the same predictions for 256 CUs on the CPU."""
import functools
import sys
import time

import numpy as np
import pytest

from massivedatans_amd import _lib
from massivedatans_amd.clustering import neighbors
import region_support as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def num_cus():
    """``torch.cuda.get_device_properties(0).multi_processor_count``, asked in a child process (as tests/test_k2_rows.py
    does: torch's HIP runtime finds no device in a process where the library's runtime came first)."""
    import subprocess
    code = "import torch; print(int(torch.cuda.get_device_properties(0).multi_processor_count))"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.strip().splitlines()[-1])


def launched(which):
    return (_lib.load().mdns_profile_kernel(which) or b"").decode()


def polled(ms, points):
    """mdns_region_count_polled, which no Python wrapper reaches: the call of the native sampler's every step"""
    points = np.ascontiguousarray(points, dtype=np.float64)
    counts = np.full(len(points), -7, dtype=np.int32)
    rc = _lib.load().mdns_region_count_polled(ms._h, _lib.ptr(points), len(points), _lib.ptr(counts))
    assert rc == 0, _lib.last_error()
    return counts.astype(int)


def both_counts(ms, points, want, cus):
    """polled and plain count of the same points against ``want``, each on the instantiation the rules predict"""
    M = len(points)
    got = polled(ms, points)
    assert launched(2) == rs.count_launch(M, ms.nmembers, ms.ndim, True, cus)[0], (launched(2), M)
    assert np.array_equal(got, want), ("polled", M, np.flatnonzero(got != want)[:8])
    got = ms.count(points)
    assert launched(2) == rs.count_launch(M, ms.nmembers, ms.ndim, False, cus)[0], (launched(2), M)
    assert np.array_equal(got, want), ("plain", M, np.flatnonzero(got != want)[:8])


@functools.lru_cache(maxsize=None)
def pool_of(K, ndim, scale=1.0):
    pool = rs.hurtful_pool(K, ndim, rs.pool_rng(K, ndim), scale)
    pool.setflags(write=False)
    return pool


def probes(pool, r, n, salt=0):
    """boundary points of ``r`` first, then ``n`` points scattered over the pool's box and a little beyond"""
    rng = rs.pool_rng(len(pool), pool.shape[1], 77 + salt)
    lo, hi = pool[1:].min(axis=0) if len(pool) > 1 else pool[0], pool[1:].max(axis=0) if len(pool) > 1 else pool[0]
    span = np.where(hi > lo, hi - lo, np.abs(hi) + (hi == 0))
    with np.errstate(over="ignore"):
        scattered = lo - 0.2 * span + rng.uniform(size=(n, pool.shape[1])) * (1.4 * span)
    scattered = np.where(np.isfinite(scattered), scattered, 0.0)
    return np.ascontiguousarray(np.vstack((rs.boundary_points(pool, r), scattered)))


def counts_after_radius(ms, pool, r, cus, n=40):
    pts = probes(pool, r, n)
    both_counts(ms, pts, rs.count_within(pool, r, pts), cus)


# ===================================================================================================== A: polled count
@functools.lru_cache(maxsize=None)
def polled_case(K, ndim):
    """pool, ten packed rounds, the statement's radius for them, 40 000 points (boundary points first) and their
    counts for that radius -- and, where that radius is 0 (K = 1), for 0.4 as well"""
    pool = pool_of(K, ndim)
    chosen = rs.draw_choice(K, 10, rs.pool_rng(K, ndim, 1))
    r = rs.bootstrap_radius(pool, chosen)
    pts = probes(pool, r if r > 0 else 0.4, max(rs.POLLED_WALK))[:max(rs.POLLED_WALK)]
    want = {r: rs.count_within(pool, r, pts)}
    if not r > 0:
        want[0.4] = rs.count_within(pool, 0.4, pts)
    return pool, rs.pack(chosen), r, pts, want


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("K,ndim", rs.POLLED_SHAPES)
def test_polled_count_walks_its_staging_block(K, ndim, source, num_cus):
    """mdns_region_count_polled against the statement while M walks up and down (the staging block is replaced several
    times; 40 000 points are the throughput shape with system-scope stores), with the threshold found on the host
    (set_radius) and with the one a packed radius computation left in device memory; mdns_region_count on the same
    points gives the same counts."""
    pool, masks, r, pts, want = polled_case(K, ndim)
    ms = neighbors.MemberSet(pool)
    try:
        if source == "device":
            assert ms.bootstrap_radius_packed(masks, 10) == r
        else:
            r = r if r > 0 else 0.4
            ms.set_radius(r)
        assert 0 < want[r].sum() or r == 0
        for M in rs.POLLED_WALK:
            both_counts(ms, pts[:M], want[r][:M], num_cus)
    finally:
        ms.close()


def test_polled_count_in_a_fresh_process_grows_its_block_from_nothing(num_cus):
    """The first polled count of a process, then growth by every step of the walk: in the suite's process the staging
    block is as large as the largest call before, so only a child process sees the replacement on each growth
    ("a new block: its number so far")."""
    import json, os, subprocess, tempfile
    pool, masks, r, pts, want = polled_case(400, 3)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); from massivedatans_amd import _lib\n"
            "from massivedatans_amd.clustering import neighbors\n"
            "d = np.load(sys.argv[1]); ms = neighbors.MemberSet(d['pool']); ms.set_radius(float(d['r'])); out = []\n"
            "for M in (1, 5, 63, 257, 1000, 4000, 40000, 2, 40000):\n"
            "    p = np.ascontiguousarray(d['pts'][:M]); c = np.full(M, -7, dtype=np.int32)\n"
            "    assert _lib.load().mdns_region_count_polled(ms._h, _lib.ptr(p), M, _lib.ptr(c)) == 0, _lib.last_error()\n"
            "    out.append(c.tolist())\n"
            "print(json.dumps(out))\n" % root)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "polled.npz")
        np.savez(path, pool=pool, r=r, pts=pts)
        out = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, MDNS_POLL_TIMEOUT_S="15"))
    assert out.returncode == 0, out.stderr[-1500:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    for M, c in zip((1, 5, 63, 257, 1000, 4000, 40000, 2, 40000), got):
        assert np.array_equal(c, want[r][:M]), M


# ===================================================================================================== B: K3
def dropin_count(pool, r, pts):
    return neighbors.count_within_distance_of(pool, r, pts)


@pytest.mark.parametrize("ndim", [3, 9])
@pytest.mark.parametrize("extra", [0, 63])
def test_count_in_the_throughput_shape(extra, ndim, num_cus):
    """SL = 1 (64 points per workgroup): the first M that takes it and the last of that workgroup count, through the
    region (plain and polled: system-scope stores from 64 lanes) and through the drop-in."""
    M = rs.sl1_sizes(num_cus)[0] + extra
    pool = pool_of(70, ndim)
    r = 0.3 if ndim == 3 else 0.9
    pts = probes(pool, r, M)[:M]
    want = rs.count_within(pool, r, pts)
    assert want.max() > 0
    ms = neighbors.MemberSet(pool)
    try:
        ms.set_radius(r)
        both_counts(ms, pts, want, num_cus)
        assert launched(2) == "k_count_within<%d, 1>" % rs.dim_case(ndim)
        assert np.array_equal(dropin_count(pool, r, pts), want)
        assert launched(2) == "k_count_within<%d, 1>" % rs.dim_case(ndim)
        both_counts(ms, pts[:M - extra - 1], want[:M - extra - 1], num_cus)          # one fewer: the latency shapes again
        assert launched(2) == "k_count_within<%d, 4>" % rs.dim_case(ndim)
    finally:
        ms.close()


@pytest.mark.parametrize("M,K,ndim", rs.SPLIT_CASES)
def test_count_split_over_member_chunks(M, K, ndim, num_cus):
    """gy > 1: partial counts of member chunks (a multiple of the tile each; the last one may hold ONE member) added
    with integer atomics into a cleared buffer."""
    name, _, tile_n, gy, kchunk = rs.count_launch(M, K, ndim, False, num_cus)
    assert kchunk % tile_n == 0 and gy == (K + kchunk - 1) // kchunk
    pool = pool_of(K, ndim)
    r = 0.25 if ndim == 3 else 0.9
    pts = probes(pool, r, M)
    # the last member alone decides some counts: a point on top of it, and boundary points of it
    last = pool[-1:]
    pts = np.ascontiguousarray(np.vstack((last, rs.boundary_points(pool[::-1], r), pts)))
    for m in (M, len(pts)):
        want = rs.count_within(pool, r, pts[:m])
        assert want.max() > 1
        ms = neighbors.MemberSet(pool)
        try:
            ms.set_radius(r)
            got = ms.count(pts[:m])
            assert launched(2) == rs.count_launch(m, K, ndim, False, num_cus)[0]
            assert np.array_equal(got, want)
            assert np.array_equal(polled(ms, pts[:m]), want)
            assert np.array_equal(ms.count(pts[:m]), want)             # the cleared buffer again, after other use
        finally:
            ms.close()
        assert np.array_equal(dropin_count(pool, r, pts[:m]), want)


@functools.lru_cache(maxsize=None)
def ladder_case(K, ndim):
    """pool, a radius at the median of the distances (from the statement), points and their counts"""
    pool = pool_of(K, ndim)
    rng = rs.pool_rng(K, ndim, 5)
    base = np.ascontiguousarray(pool[rng.randint(0, K, size=21)] + rng.normal(0, 0.3, size=(21, ndim)))
    r = float(np.sqrt(np.median(rs.sq_distances(base, pool))))
    pts = np.ascontiguousarray(np.vstack((rs.boundary_points(pool, r), base)))
    return pool, r, pts, rs.count_within(pool, r, pts)


@pytest.mark.parametrize("step", rs.NDIM_LADDER)
def test_count_with_a_shrunken_member_tile(step, num_cus):
    """ndim from 14 (the last full tile of 512) up to the largest that still gets a tile of 16, K on both sides of
    the tile and one member into the third."""
    ndim = rs.ladder_ndim(step, "count")
    tile_n = rs.count_launch(5, 1, ndim, False, num_cus)[2]
    for K in (tile_n - 1, tile_n, tile_n + 1, 2 * tile_n + 1):
        pool, r, pts, want = ladder_case(K, ndim)
        assert 0 < want.sum() < want.size * K
        ms = neighbors.MemberSet(pool)
        try:
            ms.set_radius(r)
            both_counts(ms, pts, want, num_cus)
            assert launched(2) == "k_count_within<0, 4>"
        finally:
            ms.close()
        assert np.array_equal(dropin_count(pool, r, pts), want)


def test_count_refuses_an_ndim_without_a_tile(num_cus):
    """one dimension more than fits a tile of 16: a clean refusal from the drop-in, the region and the polled call,
    and a normal polled count is right afterwards"""
    ndim = rs.max_ndim("count") + 1
    assert rs.count_launch(5, 20, ndim, False, num_cus) is None
    message = rs.TILE_REFUSAL % ndim
    pool = pool_of(20, ndim)
    pts = np.ascontiguousarray(pool[:5] + 0.01)
    with pytest.raises(_lib.MdnsError, match=message):
        dropin_count(pool, 1.0, pts)
    ms = neighbors.MemberSet(pool)
    try:
        ms.set_radius(1.0)
        with pytest.raises(_lib.MdnsError, match=message):
            ms.count(pts)
        counts = np.full(5, -7, dtype=np.int32)
        assert _lib.load().mdns_region_count_polled(ms._h, _lib.ptr(pts), 5, _lib.ptr(counts)) != 0
        assert message in _lib.last_error()
        assert np.all(counts == -7)
    finally:
        ms.close()
    pool, masks, r, pts, want = polled_case(400, 3)
    ms = neighbors.MemberSet(pool)
    try:
        ms.set_radius(r)
        both_counts(ms, pts[:1000], want[r][:1000], num_cus)
    finally:
        ms.close()


# ===================================================================================================== C: K5 / K6
def check_name(K, ndim, nboot, packed, finishing, cus):
    plan = rs.nearest_launch(K, ndim, nboot, packed, finishing, cus)
    assert launched(3) == plan["windows"][-1][0], (launched(3), plan)
    return plan


@functools.lru_cache(maxsize=None)
def rounds_case(K, ndim, nboot):
    pool = pool_of(K, ndim)
    chosen = rs.draw_choice(K, nboot, rs.pool_rng(K, ndim, nboot))
    return pool, chosen, rs.bootstrap_radius(pool, chosen)


@pytest.mark.parametrize("nboot", rs.ROUND_COUNTS)
@pytest.mark.parametrize("K,ndim", rs.F64_POOLS)
def test_f64_choice_in_round_windows(K, ndim, nboot, num_cus):
    """The f64 choice matrix through the region (K <= 2048: the kernel reads the matrix itself; above: k_pack_chosen
    per window of 16) and through the non-finishing drop-in (always k_pack_chosen), at the RT boundary 10 | 11, a full
    window, a window of one round behind a full one, two full windows and a third of one round (from 17 rounds on
    the region takes a round buffer of its own)."""
    pool, chosen, want = rounds_case(K, ndim, nboot)
    assert 0 < want < 1e100
    ms = neighbors.MemberSet(pool)
    try:
        assert ms.bootstrap_radius(chosen) == want
        plan = check_name(K, ndim, nboot, False, True, num_cus)
        assert plan["fused"] == (K <= rs.FUSED_MOST) and plan["own_rounds"] == (nboot > rs.SLOT_ROUNDS)
        counts_after_radius(ms, pool, want, num_cus)
        assert ms.bootstrap_radius(chosen) == want                         # on the slots the first one left
    finally:
        ms.close()
    assert neighbors.bootstrapped_maxdistance_chosen(pool, chosen) == want
    assert check_name(K, ndim, nboot, False, False, num_cus)["packs"]


@pytest.mark.parametrize("K,ndim,nboot", [(300, 3, 11), (300, 3, 10), (2049, 9, 17), (2048, 2, 33)])
def test_chosen_means_not_equal_to_zero(K, ndim, nboot, num_cus):
    """-0.0 is not chosen; 0.5, -1, a denormal and NaN are (cneighbors.c:146: != 0), on both f64 paths"""
    pool = pool_of(K, ndim)
    odd, plain = rs.odd_choice(K, nboot, rs.pool_rng(K, ndim, 3))
    for value in rs.ODD_NONZERO + (-0.0,):
        assert (np.isnan(odd).any() if value != value else ((odd == value) & (np.signbit(odd) == np.signbit(value))).any()), value
    want = rs.bootstrap_radius(pool, plain)
    assert rs.bootstrap_radius(pool, odd) == want and want > 0
    ms = neighbors.MemberSet(pool)
    try:
        with np.errstate(invalid="ignore"):
            assert ms.bootstrap_radius(odd) == want
            counts_after_radius(ms, pool, want, num_cus)
            assert ms.bootstrap_radius(plain) == want
            assert neighbors.bootstrapped_maxdistance_chosen(pool, odd) == want
    finally:
        ms.close()


@pytest.mark.parametrize("kind", rs.DEGENERATE)
@pytest.mark.parametrize("K,ndim", rs.DEGENERATE_POOLS)
def test_degenerate_rounds(K, ndim, kind, num_cus):
    """A round in which nobody is chosen (sqrt(1e300) once a point of index >= 1 exists), all chosen (0), only
    point 0 left out (0), pools of one and two points: packed and f64, region and drop-in; the counts afterwards."""
    pool = pool_of(K, ndim)
    for nboot in (10, 3, 12):
        chosen = rs.degenerate_choice(kind, K, nboot, rs.pool_rng(K, ndim, nboot))
        want = rs.bootstrap_radius(pool, chosen)
        if kind == "nobody":
            assert want == (np.sqrt(1e300) if K > 1 else 0.0)
        if kind in ("everybody", "only0_out"):
            assert want == 0.0
        ms = neighbors.MemberSet(pool)
        try:
            assert ms.bootstrap_radius_packed(rs.pack(chosen), nboot) == want
            check_name(K, ndim, nboot, True, True, num_cus)
            counts_after_radius(ms, pool, want, num_cus, n=10)
            assert ms.bootstrap_radius(chosen) == want
            check_name(K, ndim, nboot, False, True, num_cus)
            counts_after_radius(ms, pool, want, num_cus, n=10)
        finally:
            ms.close()
        assert neighbors.bootstrapped_maxdistance_chosen(pool, chosen) == want
    assert neighbors.most_distant_nearest_neighbor(pool) == rs.nn_radius(pool)


@pytest.mark.parametrize("nboot", rs.GARBAGE_ROUNDS)
@pytest.mark.parametrize("K,ndim", rs.GARBAGE_POOLS)
def test_packed_masks_with_garbage_above_the_rounds(K, ndim, nboot, num_cus):
    """bits nboot..15 of the packed masks set at random (bits 16..31 are zero: include/mdns.h): the kernels carry 10
    or 16 rounds and must keep the unused ones out of the max"""
    pool = pool_of(K, ndim)
    rng = rs.pool_rng(K, ndim, 100 + nboot)
    chosen = rs.draw_choice(K, nboot, rng)
    masks = rs.with_garbage(rs.pack(chosen), nboot, rng)
    assert (masks >> np.uint32(nboot)).any() and not (masks >> np.uint32(16)).any()
    # were the garbage rounds counted the radius would be another one
    wide = ((masks[:, None] >> np.arange(16, dtype=np.uint32)[None, :]) & 1).astype(float)
    want = rs.bootstrap_radius(pool, chosen)
    assert rs.bootstrap_radius(pool, wide) == np.sqrt(1e300) != want
    ms = neighbors.MemberSet(pool)
    try:
        assert ms.bootstrap_radius_packed(masks, nboot) == want
        check_name(K, ndim, nboot, True, True, num_cus)
        assert ms.bootstrap_radius_packed(rs.pack(chosen), nboot) == want
        counts_after_radius(ms, pool, want, num_cus)
    finally:
        ms.close()
    ms, got = neighbors.MemberSet.bootstrapped(pool, masks, nboot)
    ms.close()
    assert got == want


@pytest.mark.parametrize("step", rs.NDIM_LADDER)
def test_radii_with_a_shrunken_member_tile(step, num_cus):
    """K5, K6 packed (10 rounds) and K6 f64 (11 rounds: 16 carried) up the ndim ladder, each to its own largest ndim,
    with 40 points and with one point more than the shrunken tile holds"""
    for kind, nboot in (("nearest", None), ("bootstrap", 10), ("bootstrap", 11)):
        ndim = rs.ladder_ndim(step, kind, nboot)
        plan = rs.nearest_launch(40, ndim, nboot, nboot == 10, True, num_cus)
        tile_n = plan["windows"][0][1]
        assert tile_n < rs.MAX_TILE or step == 14
        for K in (40, tile_n + 1):
            pool = pool_of(K, ndim)
            if kind == "nearest":
                assert neighbors.most_distant_nearest_neighbor(pool) == rs.nn_radius(pool)
                assert launched(3) == "k_nearest_chosen<0, true, 4, 10>"
                continue
            chosen = rs.draw_choice(K, nboot, rs.pool_rng(K, ndim, nboot))
            want = rs.bootstrap_radius(pool, chosen)
            assert want > 0
            ms = neighbors.MemberSet(pool)
            try:
                if nboot == 10:
                    assert ms.bootstrap_radius_packed(rs.pack(chosen), nboot) == want
                    assert launched(3) == "k_nearest_chosen<0, false, 4, 10>"
                else:
                    assert ms.bootstrap_radius(chosen) == want
                    assert launched(3) == "k_nearest_chosen<0, false, 4, 16>"
                counts_after_radius(ms, pool, want, num_cus, n=10)
            finally:
                ms.close()
            assert neighbors.bootstrapped_maxdistance_chosen(pool, chosen) == want


def test_radii_refuse_an_ndim_without_a_tile(num_cus):
    """above the largest ndim the radius comes back NaN and the wrappers raise with the tile message; the handle
    computes a radius of fewer rounds (less LDS beside the tile) afterwards"""
    ndim = rs.max_ndim("nearest") + 1
    with pytest.raises(_lib.MdnsError, match=rs.TILE_REFUSAL % ndim):
        neighbors.most_distant_nearest_neighbor(pool_of(20, ndim))
    ndim = rs.max_ndim("bootstrap", 11) + 1
    assert ndim <= rs.max_ndim("bootstrap", 10)
    pool = pool_of(20, ndim)
    chosen11 = rs.draw_choice(20, 11, rs.pool_rng(20, ndim, 11))
    ms = neighbors.MemberSet(pool)
    try:
        with pytest.raises(_lib.MdnsError, match=rs.TILE_REFUSAL % ndim):
            ms.bootstrap_radius(chosen11)
        with pytest.raises(_lib.MdnsError, match=rs.TILE_REFUSAL % ndim):
            ms.bootstrap_radius_packed(rs.pack(chosen11), 11)
        assert ms.bootstrap_radius(chosen11[:, :10]) == rs.bootstrap_radius(pool, chosen11[:, :10])
        assert ms.bootstrap_radius_packed(rs.pack(chosen11[:, :9]), 9) == rs.bootstrap_radius(pool, chosen11[:, :9])
    finally:
        ms.close()
    with pytest.raises(_lib.MdnsError, match=rs.TILE_REFUSAL % ndim):
        neighbors.bootstrapped_maxdistance_chosen(pool, chosen11)
    ndim = rs.max_ndim("bootstrap", 10) + 1
    with pytest.raises(_lib.MdnsError, match=rs.TILE_REFUSAL % ndim):
        neighbors.bootstrapped_maxdistance_chosen(pool_of(20, ndim), rs.draw_choice(20, 3, rs.pool_rng(20, ndim)))


@pytest.mark.parametrize("K,ndim", rs.PACKED_LARGE)
def test_packed_choice_on_large_pools(K, ndim, num_cus):
    """Packed masks at K >= 640: k_nearest_uniform where its member chunks are ragged (641: chunks of 132 and a last
    of 113; 8193: chunks of 516 = tiles of 512 + 4), and above 5 dimensions k_nearest_chosen on packed masks."""
    pool = pool_of(K, ndim)
    ms = neighbors.MemberSet(pool)
    try:
        # (the statement of 8193 points takes a second and a half: one round count per pool there)
        for nboot in ((10, 16, 3) if K < 8000 else ((10,) if ndim == 3 else (16,))):
            chosen = rs.draw_choice(K, nboot, rs.pool_rng(K, ndim, nboot))
            want = rs.bootstrap_radius(pool, chosen)
            assert ms.bootstrap_radius_packed(rs.pack(chosen), nboot) == want
            plan = check_name(K, ndim, nboot, True, True, num_cus)
            assert (plan["uniform"] is not None) == (ndim <= 5)
        counts_after_radius(ms, pool, want, num_cus)
    finally:
        ms.close()


@pytest.fixture(scope="module")
def sl1_cases(num_cus, oracle):
    """The two pools of the throughput shape (ndim 3), three rounds each, with the C oracle's radii: the full matrix of
    squared distances would be 8.6 GB for the statement.  (The oracle is compared with the statement bit for bit in
    tests/test_region_shapes_host.py.)"""
    from oracle.oracle import Oracle
    try:
        threaded = Oracle("port-omp")                           # one thread per round
    except OSError:
        threaded = oracle
    cases = []
    for K in rs.sl1_sizes(num_cus):
        pool = pool_of(K, 3)
        chosen = np.ascontiguousarray(rs.draw_choice(K, 3, rs.pool_rng(K, 3, 3)))
        t0 = time.perf_counter()
        k6 = threaded.bootstrapped_maxdistance(pool, chosen)
        t1 = time.perf_counter()
        k5 = oracle.most_distant_nearest_neighbor(pool) if K == rs.sl1_sizes(num_cus)[0] else None
        print("SL = 1 reference, K = %d: K6 3 rounds %.2f s, K5 %.2f s" % (K, t1 - t0, time.perf_counter() - t1))
        cases.append(dict(K=K, pool=pool, chosen=chosen, k6=k6, k5=k5))
    # packed masks take k_nearest_uniform up to 5 dimensions: with 6, SL = 1 of k_nearest_chosen on packed masks
    K = rs.sl1_sizes(num_cus)[0]
    cases[0]["pool6"] = pool_of(K, 6)
    cases[0]["k6_6"] = threaded.bootstrapped_maxdistance(cases[0]["pool6"], cases[0]["chosen"])
    return cases


@pytest.mark.parametrize("which", [0, 1])
def test_radii_in_the_throughput_shape(which, sl1_cases, num_cus):
    """SL = 1 (K5/K6 take it from ceil(K / 64) >= 2 CUs on): K5 once, K6 with three rounds packed and f64, and the
    counts of the boundary points afterwards."""
    case = sl1_cases[which]
    K, pool = case["K"], case["pool"]
    t0 = time.perf_counter()
    if case["k5"] is not None:
        assert neighbors.most_distant_nearest_neighbor(pool) == case["k5"]
        assert launched(3) == "k_nearest_chosen<3, true, 1, 10>"
    ms = neighbors.MemberSet(pool)
    try:
        assert ms.bootstrap_radius(case["chosen"]) == case["k6"]
        assert launched(3) == "k_nearest_chosen<3, false, 1, 10>"
        assert launched(3) == rs.nearest_launch(K, 3, 3, False, True, num_cus)["windows"][-1][0]
        counts_after_radius(ms, pool, case["k6"], num_cus)
        assert ms.bootstrap_radius_packed(rs.pack(case["chosen"]), 3) == case["k6"]
        check_name(K, 3, 3, True, True, num_cus)
        counts_after_radius(ms, pool, case["k6"], num_cus)
    finally:
        ms.close()
    assert neighbors.bootstrapped_maxdistance_chosen(pool, case["chosen"]) == case["k6"]
    assert launched(3) == "k_nearest_chosen<3, false, 1, 10>"
    if "pool6" in case:
        ms, got = neighbors.MemberSet.bootstrapped(case["pool6"], rs.pack(case["chosen"]), 3)
        try:
            assert got == case["k6_6"]
            assert launched(3) == "k_nearest_chosen<6, false, 1, 10>"
            counts_after_radius(ms, case["pool6"], got, num_cus)
        finally:
            ms.close()
    print("SL = 1, K = %d: device side of the test %.2f s" % (K, time.perf_counter() - t0))


@pytest.mark.parametrize("scale", rs.SCALES)
def test_radius_and_threshold_at_extreme_scales(scale, num_cus):
    """Squared distances that are denormal (1e-160), tiny, ordinary, around the 1e300 seed (1e150) and infinite
    (3e153): the radius, then the counts with the threshold the device derived (its full bisection below 1e-300 and
    above 1e300) and with the host's after set_radius."""
    K, ndim, nboot = 50, 2, 10
    pool = pool_of(K, ndim, scale)
    chosen = rs.draw_choice(K, nboot, rs.pool_rng(K, ndim, nboot))
    want = rs.bootstrap_radius(pool, chosen)
    d = rs.sq_distances(pool[1:], pool[1:])
    if scale == 1e-160:
        assert 0 < d.max() < 2.3e-308 and 0 < want < 1e-159
    nn = rs.nn_radius(pool)
    if scale == 1e150:                       # point 0 is further than the seed from everybody: K5 answers the seed
        assert 1e140 < want < 1e150 and nn == 1e150 and (rs.sq_distances(pool[:1], pool[1:]) > 1e300).all()
    if scale == 3e153:
        assert want == 1e150 and nn == 1e150 and (d > 1e300).any() and np.isinf(rs.sq_distances(pool[:1], pool[1:])).all()
    pts = probes(pool, want, 40)
    counts = rs.count_within(pool, want, pts)
    assert 0 < counts.sum() or scale == 3e153
    ms = neighbors.MemberSet(pool)
    try:
        assert ms.bootstrap_radius_packed(rs.pack(chosen), nboot) == want
        both_counts(ms, pts, counts, num_cus)                           # the device's threshold
        ms.set_radius(want)
        both_counts(ms, pts, counts, num_cus)                           # the host's
        assert ms.bootstrap_radius(chosen) == want
        both_counts(ms, pts, counts, num_cus)
        if nn > 0:
            ms.set_radius(nn)
            both_counts(ms, pts, rs.count_within(pool, nn, pts), num_cus)
    finally:
        ms.close()
    assert neighbors.bootstrapped_maxdistance_chosen(pool, chosen) == want
    assert neighbors.most_distant_nearest_neighbor(pool) == nn
    assert np.array_equal(dropin_count(pool, want, pts), counts)


# ===================================================================================================== D: one handle
def test_one_handle_through_many_computations(num_cus):
    """Packed, f64 with a round buffer of its own, packed again, a set radius, f64 in the slab's slots' successor,
    an all-chosen choice and the first masks again on ONE region -- every finishing computation must leave the round
    slots and tickets zero for whichever kind comes next -- each followed by a polled and a plain count; then the same
    on a second region created while the first is alive (neighbouring result slots)."""
    K, ndim = 700, 3
    pool = pool_of(K, ndim)
    c10, c33, c16, c11 = (rs.draw_choice(K, n, rs.pool_rng(K, ndim, 200 + n)) for n in (10, 33, 16, 11))
    r10, r33, r16, r11 = (rs.bootstrap_radius(pool, c) for c in (c10, c33, c16, c11))
    assert len({r10, r33, r16, r11}) >= 3 and min(r10, r33, r16, r11) > 0
    every = np.ones((K, 10))

    def counted(ms, r):
        pts = probes(pool, r, 60)
        both_counts(ms, pts, rs.count_within(pool, r, pts), num_cus)

    def sequence(ms):
        assert ms.bootstrap_radius_packed(rs.pack(c10), 10) == r10
        assert launched(3) == "k_nearest_uniform<3, 10>"
        counted(ms, r10)
        assert ms.bootstrap_radius(c33) == r33
        assert rs.nearest_launch(K, ndim, 33, False, True, num_cus)["own_rounds"]
        counted(ms, r33)
        assert ms.bootstrap_radius_packed(rs.pack(c16), 16) == r16
        assert launched(3) == "k_nearest_uniform<3, 16>"
        counted(ms, r16)
        ms.set_radius(0.5 * r16)
        counted(ms, 0.5 * r16)
        assert ms.bootstrap_radius(c11) == r11
        assert launched(3) == "k_nearest_chosen<3, false, 4, 16>"
        counted(ms, r11)
        assert ms.bootstrap_radius(every) == 0.0
        pts = probes(pool, r10, 60)
        both_counts(ms, pts, np.zeros(len(pts), dtype=int), num_cus)
        assert ms.bootstrap_radius_packed(rs.pack(c10), 10) == r10
        counted(ms, r10)

    first = neighbors.MemberSet(pool)
    try:
        sequence(first)
        second = neighbors.MemberSet(pool)
        try:
            sequence(second)
            assert first.bootstrap_radius_packed(rs.pack(c16), 16) == r16       # the first one is still whole
            counted(first, r16)
        finally:
            second.close()
    finally:
        first.close()
