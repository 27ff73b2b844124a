"""Test helpers of the K2 matrix-core filter (csrc/mdns_k2gemm.hip; test_k2_filter_shapes.py, k2_filter_cases.py):
the configurations and their children, the shape list, the input builder, a plain statement of the filter in
``np.longdouble`` with the classes of outcome it allows, and the rule that names the kernel instantiation.

The statement, for spectra y, variances v, templates m [B][nx], thresholds thr [ndata], bounds bound [B]:

    w    = 1 / v                      (rounded to double as the upload does, then exact)
    A_d  = sum_j y^2 w
    s    = sum_j y w m / (1e-10 + sum_j w m^2)
    Lq   = -1/2 sum_j (y - s m)^2 w                        (the residual form: nothing cancels)
    band = 1.01 bound[b] + 1e-12 (|Lq| + |thr_d|) + gamma A_d,   gamma = 32 (nx + 16) 2^-52

The kernel computes the expanded form Lf = -1/2 (A - 2 s S1 + s^2 S2); csrc/mdns_k2gemm.hip states a first-order
rounding bound of about 4 (nx + 16) u A for it and widens its band by E = gamma A = 32 (nx + 16) u A, u = 2^-52.
The slack these tests grant is S = gamma A_d / 4 = 8 (nx + 16) u A_d: twice the stated first-order bound, a quarter
of E -- derived, not measured.  With it a selected pair

    must clear       when  Lq - thr >   band + S
    must be silent   when  Lq - thr < -(band + S)
    must be listed   when |Lq - thr| <  band - S      (or Lq is not finite)
    is a sliver      otherwise: either outcome is allowed

and the inputs are chosen so that there are no slivers at all (asserted without a GPU)."""
import os

import numpy as np

from massivedatans_amd import gen
import filter_support as fs

ROOT = fs.ROOT
GAMMA_FACTOR = 32.0 * 2.0 ** -52

#: configuration -> what the child's environment adds; the library reads MDNS_K2_FILTER_* once per process
CONFIGS = {
    "default": {},
    "P=1": {"MDNS_K2_FILTER_P": "1"},            # one workgroup walks every tile: red is reused
    "P=3": {"MDNS_K2_FILTER_P": "3"},
    "P=7": {"MDNS_K2_FILTER_P": "7"},
    "P=1000": {"MDNS_K2_FILTER_P": "1000"},      # more workgroups than units at the small shapes; pieces inside a tile
    "P=0": {"MDNS_K2_FILTER_P": "0"},            # one workgroup per tile, never split
    "TILED=0": {"MDNS_K2_FILTER_TILED": "0"},
    "SK=0": {"MDNS_K2_FILTER_SK": "0"},
    "SK=0,KW=4": {"MDNS_K2_FILTER_SK": "0", "MDNS_K2_FILTER_KW": "4"},
    "SK=0,KW=8": {"MDNS_K2_FILTER_SK": "0", "MDNS_K2_FILTER_KW": "8"},
    "NC=1": {"MDNS_K2_FILTER_NC": "1"},
    "NC=4": {"MDNS_K2_FILTER_NC": "4"},
}
_SWITCHES = ("MDNS_K2_FILTER", "MDNS_K2_FILTER_P", "MDNS_K2_FILTER_TILED", "MDNS_K2_FILTER_SK", "MDNS_K2_FILTER_KW",
             "MDNS_K2_FILTER_NC")
#: the configuration of this process if it is a child of test_k2_filter_shapes.py
CONFIG_VARIABLE = "MDNS_TEST_K2_CONFIG"
#: where the children of one session keep the references they share
CACHE_VARIABLE = "MDNS_TEST_K2_CACHE"
#: the repeated launches of Part C run where the hand-over between workgroups is busiest
REPEAT_CONFIGS = ("P=7", "P=1000")
REPEATS = 100


def child_environment(config, cache=None):
    """Environment of the child that runs under ``config``: every MDNS_K2_FILTER* of the caller's removed, the
    configuration's own added."""
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env.update(CONFIGS[config])
    env[CONFIG_VARIABLE] = config
    if cache is not None:
        env[CACHE_VARIABLE] = str(cache)
    return env


def run_child(config, path, cache=None, timeout=600):
    """One child pytest over ``path`` under ``config`` (filter_support.run_child with this module's environment:
    once, never again, and not at all after a child of the session died)."""
    return fs.run_child(config, path, cache=cache, timeout=timeout, environment=child_environment)


# ---------------------------------------------------------------------------------------
# which instantiation launch_muse_filter picks
# ---------------------------------------------------------------------------------------
#: compute units of the MI355X: the whole-tile family takes 4 waves from 3 tiles per unit on, which no shape here reaches
NUM_CUS = 256


def expected_kernel(config, ndata, nx, B, rows, M):
    """The name ``mdns_profile_kernel(1)`` must report after a pass over ``M`` selected spectra (``rows``: their ids or
    None) of ``ndata`` x ``nx`` with ``B`` candidates under ``config``, restated from launch_muse_filter: NC by B (1 up
    to 16 candidates, 2 up to 32, 4 above) unless forced; operands tiled only without rows and with M == ndata; of the
    whole-tile family 8 waves, 4 when forced or when there are fewer than 16 channel groups."""
    env = CONFIGS[config]
    nc = int(env.get("MDNS_K2_FILTER_NC", 4 if B > 32 else (2 if B > 16 else 1)))
    if env.get("MDNS_K2_FILTER_SK") != "0":
        tiled = rows is None and M == ndata and env.get("MDNS_K2_FILTER_TILED") != "0"
        return "k_muse_gemm_band_sk<%d, tiled>" % nc if tiled else "k_muse_gemm_band_sk<%d>" % nc
    tiles = ((M + 15) // 16) * ((B + 16 * nc - 1) // (16 * nc))
    assert tiles < 3 * NUM_CUS, "a shape this large takes 4 waves by itself: restate the rule"
    kw = int(env.get("MDNS_K2_FILTER_KW", 8))
    if (nx + 15) // 16 < 16:
        kw = 4
    return "k_muse_gemm_band<%d, %d>" % (nc, kw)


# ---------------------------------------------------------------------------------------
# shapes, inputs
# ---------------------------------------------------------------------------------------
#: (ndata, nx, B, selection, seed).  selection: None = every spectrum; "third" = an ascending random third with row 0
#: and row ndata - 1; ("prefix", M) = rows None with M < ndata (row-major by the prefix rule); ("tenth", M) = M random
#: rows.  The seed is the one at which the reference yields no sliver and every class of outcome (see ``Case.check``).
SHAPES = [
    (1, 1, 1, None, 0),                   # one channel group, one lane of work
    (15, 16, 8, None, 0),
    (17, 17, 16, None, 4),                # ng 1 -> 2; row tile ragged
    (33, 40, 17, None, 0),                # NC = 2, second candidate tile nearly empty
    (100, 255, 32, None, 0),
    (100, 256, 33, None, 0),              # NC = 4 with a 1-candidate last tile
    (100, 257, 57, None, 0),              # ng = 17: one past the loop's 2 KW stride
    (250, 300, 64, None, 0),
    (250, 700, 65, None, 0),              # bt = 2; ng = 44 is not a multiple of 8
    (64, 4096, 64, None, 0),              # the benchmark's channel count; ng = 256
    (130, 520, 130, None, 0),
    (250, 700, 40, "third", 0),
    (250, 300, 64, ("prefix", 200), 0),
    (500, 333, 9, ("tenth", 50), 0),
    (100, 256, 5, None, 0),               # under NC=4: three of four candidate tiles are clamps
]
#: Part C walks these in this order -- small, large, small -- in ONE process, so that the scratch of the hand-over and
#: the tiled template buffer grow and are then reused with stale columns past B
ORDER_C = [1, 3, 8, 9, 10, 2, 0, 14]
REPEAT_SHAPE = 8                          # 250 x 700 x 65
#: the threshold offsets in units of the band, ordered listed, clear, silent, ...: any three in a row hold all classes
OFFSETS = np.array([0.0, -1.5, 1.5, 0.5, -10.0, 10.0, -0.5, -1e6, 1e6])
#: launches of a case: with the all-zero bound over the spectra that hold a NaN, with the graded bound over the plain ones
DRAWS = 4


def shape_id(shape):
    ndata, nx, B, sel, _ = shape
    return "%dx%dx%d-%s" % (ndata, nx, B, "all" if sel is None else (sel if isinstance(sel, str) else "%s%d" % sel))


def selection(shape, rng):
    """(rows or None, M)"""
    ndata, _, _, sel, _ = shape
    if sel is None:
        return None, ndata
    if sel == "third":
        inner = rng.choice(np.arange(1, ndata - 1), size=ndata // 3 - 2, replace=False)
        rows = np.sort(np.concatenate([[0, ndata - 1], inner])).astype(np.int32)
        return rows, len(rows)
    kind, M = sel
    if kind == "prefix":
        return None, M
    return np.sort(rng.choice(ndata, size=M, replace=False)).astype(np.int32), M


def bench_like_params(rng, B):
    """The five parameters of B templates, drawn as bench.py draws them."""
    return np.column_stack([rng.uniform(-0.3, 0.3, B), rng.uniform(0.0, 0.02, B), rng.uniform(-0.2, 0.2, B),
                            rng.uniform(0.5, 1.5, B), rng.uniform(0.5, 1.5, B)])


#: a template no spectrum resembles (lines ten times the continuum and thirty times as wide -- they show on the
#: coarsest grid here --, at a redshift nobody has): the candidate every other one beats everywhere, so that some
#: candidate can be silent
POOR_TEMPLATE = (1.0, 0.06, 1.5, 3.0, 3.0)


class Case(object):
    """Inputs of one shape: ``gen.muse_like`` spectra, every third multiplied by 1e3 (A grows 1e6-fold: the term
    gamma A then dwarfs 1e-12 (|L| + |thr|), and Lf is the small difference of terms that large wherever a template
    fits), one spectrum of the selection with a NaN channel in the ``y_nan`` copy, templates from
    ``gen.muse_template`` with bench.py's parameter ranges and, from two candidates on, POOR_TEMPLATE in the middle."""

    def __init__(self, shape):
        ndata, nx, B, _, seed = shape
        self.shape, self.ndata, self.nx, self.B = shape, ndata, nx, B
        rng = np.random.RandomState(100003 * seed + 1000 * nx + 7 * ndata + B)
        data = gen.muse_like(ndata, nx)
        self.x = data["x"]
        y = np.array(data["y"])
        y[:, np.arange(ndata) % 3 == 1] *= 1e3
        self.y, self.v = np.ascontiguousarray(y), np.ascontiguousarray(data["v"])
        self.params = bench_like_params(rng, B)
        if B > 1:
            self.params[B // 2] = POOR_TEMPLATE
        self.templates = np.ascontiguousarray([gen.muse_template(self.x, p) for p in self.params])
        self.rows, self.M = selection(shape, rng)
        self.sel = np.arange(self.M) if self.rows is None else self.rows
        self.d_nan = int(self.sel[len(self.sel) // 2])
        self.y_nan = self.y.copy()
        self.y_nan[nx // 2, self.d_nan] = np.nan
        self.owner_offset = rng.randint(len(OFFSETS), size=B)
        self.draw_seed = int(rng.randint(1 << 30))
        self.gamma = GAMMA_FACTOR * (nx + 16)

    # ---- the statement ----
    def reference(self):
        """(A [ndata], Lq [B, ndata]) in np.longdouble for the plain spectra, once per session (the children share
        it on disk)."""
        if getattr(self, "_ref", None) is None:
            cache = os.environ.get(CACHE_VARIABLE)
            path = os.path.join(cache, shape_id(self.shape) + "-%d.npz" % self.shape[4]) if cache else None
            if path and os.path.exists(path):
                with np.load(path) as f:
                    self._ref = (f["A"], f["Lq"])
            else:
                self._ref = reference_filter(self.y, self.v, self.templates)
                if path:
                    tmp = path + ".%d.tmp.npz" % os.getpid()
                    np.savez(tmp, A=self._ref[0], Lq=self._ref[1])
                    os.replace(tmp, path)
            assert self._ref[1].dtype == np.longdouble and self._ref[1].shape == (self.B, self.ndata)
        return self._ref

    def variant(self, with_nan):
        """(A, Lq) of the plain spectra, or of the copy with the NaN channel (that spectrum's column is NaN)."""
        A, Lq = self.reference()
        if with_nan:
            A, Lq = A.copy(), Lq.copy()
            A[self.d_nan] = np.nan
            Lq[:, self.d_nan] = np.nan
        return A, Lq

    def band(self, Lq, thr, bound, A):
        """band_q [B, ndata]"""
        return (np.longdouble(1.01) * bound.astype(np.longdouble).reshape(-1, 1)
                + np.longdouble(1e-12) * (np.abs(Lq) + np.abs(thr.astype(np.longdouble)).reshape(1, -1))
                + np.longdouble(self.gamma) * A.reshape(1, -1))

    def thresholds(self, A, Lq, bound, offsets):
        """float64 [ndata]: data set d gets ``Lq[d mod B, d] + offsets[d] band``; the unselected ones -1e300 (a kernel
        that indexes thr or A by position instead of by data set then votes clear), the one with the NaN 0."""
        d = np.arange(self.ndata)
        own = d % self.B
        base = Lq[own, d]
        band0 = self.band(Lq, base.astype(np.float64), bound, A)[own, d]
        thr = (base + offsets.astype(np.longdouble) * band0).astype(np.float64)
        thr[np.isnan(thr)] = 0.0
        out = np.full(self.ndata, -1e300)
        out[self.sel] = thr[self.sel]
        return out

    def launches(self, draws=DRAWS, first_draw=0):
        """The launches of the case as (with_nan, bound [B], thr [ndata]): draws 0-2 give every data set of one owner
        (candidate d mod B) the same offset, rotated by the draw -- so each candidate's own pairs are once listed,
        once clear and once silent --, later draws one offset per data set."""
        b = np.arange(self.B)
        for with_nan, bound in ((True, np.zeros(self.B)), (False, 5e-5 * (1 + b % 3))):
            A, Lq = self.variant(with_nan)
            for k in range(first_draw, first_draw + draws):
                if k < 3:
                    which = (self.owner_offset[np.arange(self.ndata) % self.B] + k) % len(OFFSETS)
                else:
                    which = np.random.RandomState(self.draw_seed + k).randint(len(OFFSETS), size=self.ndata)
                yield with_nan, bound, self.thresholds(A, Lq, bound, OFFSETS[which])

    def classify(self, with_nan, bound, thr):
        """What the statement demands of a launch: a dict of
        ``clear_must``, ``clear_may``, ``maybe_must``, ``maybe_may`` (bool [B]), ``listed``, ``slivers`` (counts) and the
        pair masks ``must_clear``, ``must_list``, ``must_silent``, ``sliver`` [B, M]."""
        A, Lq = self.variant(with_nan)
        A, Lq, t = A[self.sel], Lq[:, self.sel], thr[self.sel].astype(np.longdouble).reshape(1, -1)
        band = self.band(Lq, thr[self.sel], bound, A)
        S = np.longdouble(self.gamma) * A.reshape(1, -1) / 4
        with np.errstate(invalid="ignore"):
            diff = Lq - t
            must_clear = diff > band + S
            must_silent = diff < -(band + S)
            must_list = (np.abs(diff) < band - S) | ~np.isfinite(Lq)
        sliver = ~(must_clear | must_silent | must_list)
        upper = sliver & (diff > 0)
        return dict(must_clear=must_clear, must_silent=must_silent, must_list=must_list, sliver=sliver,
                    clear_must=must_clear.any(axis=1), clear_may=(must_clear | upper).any(axis=1),
                    maybe_must=must_list.any(axis=1), maybe_may=(must_list | sliver).any(axis=1),
                    listed=int(must_list.sum()), slivers=int(sliver.sum()))

    def check(self, clear, maybe, count, want):
        """The output of mdns_muse_filter_dev against ``classify``'s demands."""
        clear, maybe = np.asarray(clear), np.asarray(maybe)
        assert set(np.unique(clear)) <= {0, 1} and set(np.unique(maybe)) <= {0, 1}
        bad = np.flatnonzero((clear == 0) & want["clear_must"])
        assert len(bad) == 0, ("no clear vote for candidates with a pair that must clear", bad)
        bad = np.flatnonzero((clear == 1) & ~want["clear_may"])
        assert len(bad) == 0, ("a clear vote for candidates none of whose pairs may clear", bad)
        bad = np.flatnonzero((maybe == 0) & want["maybe_must"])
        assert len(bad) == 0, ("candidates with a pair that must be listed are not marked", bad)
        bad = np.flatnonzero((maybe == 1) & ~want["maybe_may"])
        assert len(bad) == 0, ("candidates marked none of whose pairs may be listed", bad)
        assert want["listed"] <= count <= want["listed"] + want["slivers"], (count, want["listed"], want["slivers"])


def reference_filter(y, v, templates):
    """``A[d]`` and ``Lq[b, d]`` of the module's statement in np.longdouble; y and v are [nx, ndata], templates [B, nx]."""
    yl = np.asarray(y, dtype=np.float64).T.astype(np.longdouble)                  # [ndata, nx]
    w = (1.0 / np.asarray(v, dtype=np.float64)).T.astype(np.longdouble)            # the upload's division, then exact
    m = np.asarray(templates, dtype=np.float64).astype(np.longdouble)
    A = (yl * yl * w).sum(axis=1)
    yw = yl * w
    Lq = np.empty((len(m), len(yl)), dtype=np.longdouble)
    for b in range(len(m)):
        mb = m[b].reshape(1, -1)
        s = (yw * mb).sum(axis=1) / (np.longdouble(1e-10) + (w * mb * mb).sum(axis=1))
        r = yl - s.reshape(-1, 1) * mb
        Lq[b] = np.longdouble(-0.5) * (r * r * w).sum(axis=1)
    return A, Lq


def preconditions(case, draws=DRAWS, first_draw=0):
    """Over all launches of a case, on the reference alone: (sliver pairs, selected pairs, launches with a candidate
    that must clear, with a listed pair, with a candidate that must stay silent -- neither vote nor mark)."""
    slivers = pairs = clear = listed = silent = 0
    for with_nan, bound, thr in case.launches(draws, first_draw):
        want = case.classify(with_nan, bound, thr)
        slivers += want["slivers"]
        pairs += want["sliver"].size
        clear += bool(want["clear_must"].any())
        listed += bool(want["listed"] > 0)
        silent += bool((~want["clear_may"] & ~want["maybe_may"]).any())
    return slivers, pairs, clear, listed, silent
