"""What the shape tests of the RadFriends region kernels share (tests/test_region_shapes*.py); no device here.

Three things: the plain statement of K3 / K5 / K6 in numpy float64 (independent of the C oracle, compared with it bit
for bit on the CPU); the launch rules of csrc/mdns_neighbors.hip restated as pure functions, so that every GPU case
can be asserted -- on the CPU -- to reach the instantiation and geometry it was built for; and the case builders.

Everything is exact: counts are integers and radii are bit-identical doubles by construction (separate multiply and
add over ascending dimensions, then only min / max selections and one correctly rounded square root)."""
import numpy as np

SEED = 1e300                 # cneighbors.c:51,148: the "no neighbour yet" squared distance

# ---------------------------------------------------------------------------------------------------------------
# the plain statement
# ---------------------------------------------------------------------------------------------------------------
_QUIET = dict(over="ignore", under="ignore", invalid="ignore")
_BLOCK_PAIRS = 1 << 21       # pairs per row block of the statements below (16 MB per temporary)


def sq_distances(a, b):
    """d[i, j] = |a_i - b_j|^2 summed from 0 over the dimensions in ascending order, multiply and add separate
    (numpy does not contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros((len(a), len(b)))
    with np.errstate(**_QUIET):
        for k in range(a.shape[1]):
            diff = a[:, None, k] - b[None, :, k]
            acc = acc + diff * diff
    return acc


def _row_blocks(n, width):
    step = max(1, _BLOCK_PAIRS // max(1, width))
    for lo in range(0, n, step):
        yield lo, min(n, lo + step)


def count_within(members, r, points):
    """K3 (cneighbors.c:95-119, countmax = 0): members with sqrt(d) < r, per point."""
    members, points = np.asarray(members, dtype=np.float64), np.asarray(points, dtype=np.float64)
    out = np.zeros(len(points), dtype=np.int64)
    for lo, hi in _row_blocks(len(points), len(members)):
        with np.errstate(**_QUIET):
            out[lo:hi] = (np.sqrt(sq_distances(points[lo:hi], members)) < r).sum(axis=1)
    return out


def nn_radius(points):
    """K5 (cneighbors.c:47-71): max over the points of the distance to the nearest OTHER point, the squared minimum
    seeded with 1e300."""
    points = np.asarray(points, dtype=np.float64)
    K = len(points)
    worst = 0.0
    for lo, hi in _row_blocks(K, K):
        d = sq_distances(points[lo:hi], points)
        d[np.arange(hi - lo), np.arange(lo, hi)] = np.inf                      # j != i
        worst = max(worst, float(np.minimum(SEED, d.min(axis=1)).max()))
    return float(np.sqrt(worst))


def bootstrap_radius(points, chosen):
    """K6 (cneighbors.c:137-176): per round the max, over the left-out points of index >= 1, of
    min(1e300, min over the chosen); the max over the rounds seeded with 0; the square root after the max."""
    points, chosen = np.asarray(points, dtype=np.float64), np.asarray(chosen, dtype=np.float64)
    K, nboot = chosen.shape
    with np.errstate(invalid="ignore"):
        sel = chosen != 0                                                       # NaN != 0: chosen
    best = 0.0
    for lo, hi in _row_blocks(K, K):
        d = sq_distances(points[lo:hi], points)
        rows = np.arange(lo, hi)
        for b in range(nboot):
            out = (~sel[lo:hi, b]) & (rows >= 1)
            if not out.any():
                continue
            cols = sel[:, b]
            nearest = np.minimum(SEED, d[out][:, cols].min(axis=1)) if cols.any() else np.full(int(out.sum()), SEED)
            best = max(best, float(nearest.max()))
    return float(np.sqrt(best))


# ---------------------------------------------------------------------------------------------------------------
# the launch rules of csrc/mdns_neighbors.hip, restated
# ---------------------------------------------------------------------------------------------------------------
MAX_TILE = 512               # kMaxTile
ROUNDS = 16                  # kRounds: rounds per window, and the most a packed choice holds
LDS_BUDGET = 60 * 1024       # kLdsBudget
MAX_REG_DIM = 8              # the largest case of MDNS_DIM_SWITCH; above it D = 0 (runtime ndim)
SLOT_ROUNDS = 16             # kSlotRounds (mdns_core.hip): more rounds than this and a region takes a round buffer of its own
FUSED_MOST = 2048            # a finishing f64 computation on at most this many points reads the choice matrix itself
UNIFORM_LEAST = 640          # packed choices, 1..5 dimensions, at least this many points: k_nearest_uniform
TILE_REFUSAL = "ndim=%d too large for the member tile"


def pick_tile(ndim, per_member_extra, fixed_bytes):
    per = ndim * 8 + per_member_extra
    if fixed_bytes + 16 * per > LDS_BUDGET:
        return 0
    return min((LDS_BUDGET - fixed_bytes) // per, MAX_TILE) & ~15


def dim_case(ndim):
    return ndim if ndim <= MAX_REG_DIM else 0


def _small(n, cus):
    return (n + 63) // 64 < 2 * cus


def count_launch(M, K, ndim, mail, cus):
    """launch_count_within: (name, pts, tile_n, gy, kchunk); None where the launch is refused (TILE_REFUSAL)."""
    tile_n = pick_tile(ndim, 0, 4 * 64 * 4)
    if tile_n <= 0:
        return None
    small = _small(M, cus)
    pts = 4 if (mail and small) else (16 if small else 64)
    gx = (M + pts - 1) // pts
    gy = min((2 * cus + gx - 1) // gx, (K + tile_n - 1) // tile_n)
    if mail:
        gy = 1
    gy = min(max(gy, 1), 65535)
    kchunk = (K + gy - 1) // gy
    kchunk = (kchunk + tile_n - 1) // tile_n * tile_n
    gy = (K + kchunk - 1) // kchunk
    return "k_count_within<%d, %d>" % (dim_case(ndim), 64 // pts), pts, tile_n, gy, kchunk


def _nearest_fixed(nboot, small):
    """bytes of the partial minima [4 waves][rounds carried][points per workgroup]; nboot None: K5"""
    carried = 1 if nboot is None else (ROUNDS if nboot > 10 else 10)
    return 4 * carried * (16 if small else 64) * 8


def nearest_launch(K, ndim, nboot, packed, finishing, cus):
    """launch_nn_maxsq (nboot None), launch_bootstrap (packed False) and launch_bootstrap_packed (packed True):
    a dict with ``windows`` = [(name, tile_n)] per window of 16 rounds (the name mdns_profile_kernel(3) reports after
    the LAST window is windows[-1][0]), ``fused`` (the kernel reads the f64 matrix itself), ``packs`` (k_pack_chosen
    runs per window), ``own_rounds`` (a region takes a round buffer of its own) and, for the uniform path,
    ``uniform`` = (ny, kchunk, tile_n).  None where the launch is refused (TILE_REFUSAL)."""
    nn = nboot is None
    assert not (packed and (nn or nboot > ROUNDS or not finishing))
    if packed and 1 <= ndim <= 5 and K >= UNIFORM_LEAST:
        rt = 10 if nboot <= 10 else ROUNDS
        gy = min(max(K // 128, 1), 16)
        kchunk = ((K + gy - 1) // gy + 3) & ~3
        ny = (K + kchunk - 1) // kchunk
        tile_n = pick_tile(ndim, 4, 4 * rt * 64 * 8)
        if tile_n <= 0:
            return None
        if tile_n > kchunk:
            tile_n = (kchunk + 15) & ~15
        return dict(windows=[("k_nearest_uniform<%d, %d>" % (ndim, rt), tile_n)], fused=False, packs=False,
                    own_rounds=False, uniform=(ny, kchunk, tile_n))
    small = _small(K, cus)
    tile_n = pick_tile(ndim, 4, _nearest_fixed(nboot, small))
    if tile_n <= 0:
        return None
    fused = (not nn) and finishing and K <= FUSED_MOST and not packed
    windows = []
    for b0 in range(0, 1 if nn else nboot, ROUNDS):
        nb = 1 if nn else min(ROUNDS, nboot - b0)
        rt = 10 if (nn or nb <= 10) else ROUNDS
        windows.append(("k_nearest_chosen<%d, %s, %d, %d>" % (dim_case(ndim), "true" if nn else "false", 4 if small else 1, rt), tile_n))
    return dict(windows=windows, fused=fused, packs=(not nn) and not fused and not packed,
                own_rounds=(not nn) and finishing and nboot > SLOT_ROUNDS, uniform=None)


def max_ndim(kind, nboot=None, small=True):
    """The largest ndim that still gets a member tile (of 16): kind "count" (K3), "nearest" (K5) or "bootstrap" (K6
    through k_nearest_chosen with ``nboot`` rounds)."""
    if kind == "count":
        extra, fixed = 0, 4 * 64 * 4
    else:
        extra, fixed = 4, _nearest_fixed(None if kind == "nearest" else nboot, small)
    ndim = 1
    while pick_tile(ndim + 1, extra, fixed) > 0:
        ndim += 1
    return ndim


def uniform_tiles(K, ndim, nboot):
    """lengths of the LDS tiles of the first and of the last member chunk of k_nearest_uniform"""
    ny, kchunk, tile_n = nearest_launch(K, ndim, nboot, True, True, 256)["uniform"]
    def tiles(n):
        return [min(tile_n, n - t) for t in range(0, n, tile_n)]
    return tiles(kchunk), tiles(K - (ny - 1) * kchunk)


# ---------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------
def hurtful_pool(K, ndim, rng, scale=1.0):
    """The pool of the K6 variant tests (a dense core in a thin halo, duplicates, a degenerate last axis, point 0 far
    outside -- it would set the radius if it counted), with a zero planted in one axis of a few members so that
    boundary_points has exactly representable differences, all times ``scale``."""
    core = rng.normal(0.5, 0.002, size=(K // 2, ndim))
    halo = rng.uniform(size=(K - K // 2, ndim))
    pts = np.vstack((core, halo))
    rng.shuffle(pts)
    if K > 7:
        pts[7] = pts[3]                                       # duplicates: distance 0 pairs
    if K > 20:
        pts[K // 3:K // 3 + min(50, K // 8)] = pts[K // 3]
    if ndim > 1:
        pts[:, ndim - 1] = 0.25                               # a degenerate axis
    for a in range(min(3, ndim - 1 if ndim > 1 else 1, K - 1)):
        pts[1 + a, a] = 0.0
    pts[0] = 7.0
    return np.ascontiguousarray(pts * scale)


def boundary_points(members, r):
    """Points whose difference from a member is r, the doubles next to r on either side, and -r along ONE axis and
    exactly zero along the others, so that the squared distance is the square of that number: sqrt(d) < r decides on
    the last bit.  Taken from the members that have a zero in the axis (the difference is then exact by
    construction) and from the first members whose sum with the difference round-trips.  The members themselves
    (distance 0) come last, so the result is never empty."""
    members = np.asarray(members, dtype=np.float64)
    out = []
    if np.isfinite(r):
        deltas = (r, np.nextafter(r, 0.0), np.nextafter(r, np.inf), -r)
        for axis in range(min(members.shape[1], 4)):
            hosts = [i for i in np.flatnonzero(members[:, axis] == 0.0)[:2]] + list(range(min(len(members), 4)))
            used = 0
            for i in hosts:
                if used == 2:
                    break
                good = []
                for delta in deltas:
                    p = members[i].copy()
                    with np.errstate(**_QUIET):
                        p[axis] = members[i, axis] + delta
                        exact = np.isfinite(p[axis]) and p[axis] - members[i, axis] == delta
                    if exact:
                        good.append(p)
                if len(good) == len(deltas):
                    out.extend(good)
                    used += 1
    out.extend(members[:3])
    return np.ascontiguousarray(np.array(out))


def draw_choice(K, nboot, rng):
    """0/1 f64[K, nboot]: per round K draws with replacement, as neighbors.draw_bootstrap_choice makes them"""
    idx = rng.randint(0, K, size=(nboot, K))
    chosen = np.zeros((K, nboot))
    chosen[idx, np.arange(nboot)[:, None]] = 1.0
    return chosen


def pack(chosen):
    """0/1 matrix of at most 16 rounds -> uint32 masks (bit b: chosen in round b)"""
    sel = np.asarray(chosen) != 0
    assert sel.shape[1] <= ROUNDS
    return np.ascontiguousarray((sel.astype(np.uint32) << np.arange(sel.shape[1], dtype=np.uint32)[None, :]).sum(axis=1), dtype=np.uint32)


def with_garbage(masks, nboot, rng):
    """random bits in nboot..13, bit 14 clear everywhere (a round in which nobody is chosen) and bit 15 set for
    member 1 alone (everybody's nearest chosen point is member 1) -- were either counted the radius would be another
    one; bits 16..31 left zero (include/mdns.h).  nboot <= 13."""
    assert nboot <= 13
    keep = np.uint32((1 << nboot) - 1)
    junk = rng.randint(0, 1 << 14, size=len(masks)).astype(np.uint32) & ~keep
    if len(masks) > 1:
        junk[1] |= np.uint32(1 << 15)
    return np.ascontiguousarray((masks & keep) | junk, dtype=np.uint32)


ODD_NONZERO = (1.0, 0.5, -1.0, 5e-324, float("nan"))


def odd_choice(K, nboot, rng):
    """(odd, plain): an f64 choice matrix whose non-zero entries are drawn from ODD_NONZERO and whose zero entries
    are 0.0 or -0.0, and the 0/1 matrix it must be equivalent to (cneighbors.c:146 tests != 0)."""
    plain = draw_choice(K, nboot, rng)
    nz = np.array(ODD_NONZERO)[rng.randint(0, len(ODD_NONZERO), size=plain.shape)]
    z = np.where(rng.randint(0, 2, size=plain.shape) == 1, -0.0, 0.0)
    odd = np.where(plain != 0, nz, z)
    return np.ascontiguousarray(odd), plain


DEGENERATE = ("nobody", "everybody", "only0_out", "mixed")


def degenerate_choice(kind, K, nboot, rng):
    """0/1 matrices with degenerate rounds: "nobody" -- one round in which nobody is chosen among ordinary ones (the
    radius is sqrt(1e300) once a point of index >= 1 exists); "everybody" -- all chosen in every round (0);
    "only0_out" -- only point 0 left out, in every round (0: point 0 never contributes); "mixed" -- ordinary rounds
    with one all-chosen round and one round that leaves out only point 0 (the radius of the ordinary rounds)."""
    chosen = draw_choice(K, nboot, rng)
    if kind == "nobody":
        chosen[:, nboot // 2] = 0.0
    elif kind == "everybody":
        chosen[:] = 1.0
    elif kind == "only0_out":
        chosen[:] = 1.0
        chosen[0] = 0.0
    elif kind == "mixed":
        chosen[:, 0] = 1.0
        chosen[:, nboot - 1] = 1.0
        chosen[0, nboot - 1] = 0.0
    else:
        raise ValueError(kind)
    return chosen


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_region_shapes.py; tests/test_region_shapes_host.py asserts, with 256 CUs, that each reaches
# the instantiation and the geometry it is meant for
# ---------------------------------------------------------------------------------------------------------------
POLLED_SHAPES = ((1, 3), (63, 2), (65, 5), (400, 3), (513, 8), (1025, 9), (300, 16))        # (K, ndim)
POLLED_WALK = (1, 3, 4, 5, 63, 257, 1000, 40000, 2)                                         # M, in this order
SPLIT_CASES = ((1, 512, 3), (1, 513, 3), (1, 1025, 3), (1, 5000, 3), (17, 5000, 3), (17, 5000, 9))   # (M, K, ndim)
SPLIT_GY = {(1, 512): 1, (1, 513): 2, (1, 1025): 3, (1, 5000): 10}
NDIM_LADDER = (14, 15, 16, 32, 100, "max")
ROUND_COUNTS = (1, 9, 10, 11, 16, 17, 32, 33)
F64_POOLS = ((300, 3), (2048, 2), (2049, 9))              # fused, fused at its limit, packed by k_pack_chosen (generic ndim)
PACKED_LARGE = ((641, 3), (641, 5), (2049, 3), (2049, 5), (8193, 3), (8193, 5), (700, 6), (700, 9))
GARBAGE_ROUNDS = (1, 3, 10, 11)
GARBAGE_POOLS = ((100, 3), (700, 3), (700, 6))
SCALES = (1e-160, 1e-30, 1.0, 1e150, 3e153)
DEGENERATE_POOLS = ((1, 3), (2, 3), (40, 3), (700, 3))


def sl1_sizes(cus):
    """the first size of the throughput shape (SL = 1) and the last of its first tile of 64"""
    first = 64 * (2 * cus - 1) + 1
    return first, first + 63


def ladder_ndim(step, kind, nboot=None):
    return max_ndim(kind, nboot) if step == "max" else step


def pool_rng(K, ndim, salt=0):
    return np.random.RandomState((K * 1009 + ndim * 31 + salt) % (2 ** 31))
