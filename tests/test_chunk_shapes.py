"""The two-launch draw chunk (csrc/mdns_chunk.hip: ``k_chunk_accept<NST>`` reading candidates and row ids from the mapped
block and computing the templates itself, then ``k_chunk_commit`` or ``k_joint_commit_trail``) at its stage, tile and
route edges, through the entry points a native constrainer calls.

1. Planted decisions per shape of ``chunk_support.CHUNK_SHAPES`` against the plain numpy statement in ``np.longdouble``
   (filter_support.py), as filter_cases.py plants them for the guarded filters -- which never reach this route.
2. Several chunks in one draw through the raw entry points against ``chunk_support.Statement``.
3. The halves (score -> votes -> commit) on this route.

After every chunk ``mdns_profile_kernel(0)`` must name the kernel ``chunk_support.expected_route`` expects: the
``k_chunk_accept<NST>`` of the stage count, or any other kernel where the chunk is to take the classic route.  Every
comparison is exact -- indices, fill bits, shelf sizes, thresholds, votes, names -- but one: the chain's likelihoods
against L_ref, at the project's RTOL_L.  The thresholds a commit leaves are compared bit for bit with the LANE kernel's
likelihoods (chain_support.LaneScorer over k_gauss_model_t's templates): a likelihood does not depend on which kernel
computed it, here with the templates k_chunk_accept makes for itself.

test_chunk_shapes_host.py shows, without a device, that the inputs keep clear of their thresholds, that the shapes
reach every branch, and that what the sequences assert occurs."""
import numpy as np
import pytest

from massivedatans_amd import _lib
from massivedatans_amd.like import GaussLineSpectra
from chain_support import LaneScorer
import chunk_support as cs
import filter_support as fs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def num_cus(hip):
    return cs.device_cus(hip)


def _kernel(hip):
    return (hip.mdns_profile_kernel(0) or b"").decode()


class _Planted(object):
    """One joint state over the spectra of a shape; ``run`` plants thresholds, draws the candidates in one chunk over
    the shape's selection and returns the outcome with the thresholds and shelf sizes afterwards."""

    def __init__(self, hip, spectra, rows, route):
        self.hip, self.rows, self.route = hip, rows, route
        self.js = cs.backend_state(spectra, cs.NLIVE)
        self.seen = set()

    def run(self, thr, params):
        live = cs.planted_live(thr)                         # (kept alive over the call: ptr is an address only)
        _lib.check(self.hip.mdns_joint_set_live(self.js._h, _lib.ptr(live)), "set_live")
        self.js.prepare()
        before, n0 = self.js.thresholds()
        assert np.array_equal(before, thr) and not n0.any()
        idx, Lrow, beats, n = self.js.draw_params(params, self.rows)
        name = _kernel(self.hip)
        cs.check_route(name, self.route)
        self.seen.add(name)
        assert n == len(params) and Lrow is None
        after, n1 = self.js.thresholds()
        return idx, beats, after, n1

    def close(self):
        self.js.close()


@pytest.mark.parametrize("shape", cs.CHUNK_SHAPES, ids=fs.shape_id)
def test_planted_decisions(hip, num_cus, shape):
    ndata, _, nx, B = shape
    M = cs.selection_size(shape)
    route = cs.expected_route(M, B, nx, num_cus)
    counts = {}
    for offset in cs.OFFSETS:
        x, y, params, rows, L_ref = cs.reference(shape, offset)
        sel = np.arange(ndata) if rows is None else rows
        assert len(sel) == M
        spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
        scorer = LaneScorer(spectra)
        # the chain's values against the plain statement, pair by pair, no allowance (test_chunk_shapes_host.py: no
        # pair of these shapes is blurred by the reference's own templates)
        Lall = scorer.loglike_batch(params)
        assert Lall.shape == (B, ndata)
        err = np.abs(Lall - L_ref) / np.abs(L_ref)
        print("%s offset %g: chain against L_ref %.3g" % (fs.shape_id(shape), offset, float(err.max())))
        assert (np.abs(Lall - L_ref) <= fs.RTOL_L * np.abs(L_ref)).all(), float(err.max())
        base = fs.unbeatable(L_ref)
        st = _Planted(hip, spectra, rows, route)
        try:
            # ordinary thresholds: some candidate is accepted, as the reference decides
            ordinary = fs.ordinary_thresholds(L_ref, rows)
            got = st.run(ordinary, params)
            cs.check_outcome(got, ordinary, rows, L_ref, Lall)
            counts["ordinary %g" % offset] = (got[0], int(got[1].sum()))
            if offset != 0.0:
                continue
            # thresholds nobody beats: index -1, thresholds and shelf sizes untouched
            got = st.run(base, params)
            assert got[0] == -1 and np.array_equal(got[2], base) and not got[3].any()
            cs.check_outcome(got, base, rows, L_ref, Lall)
            # thresholds ON the chain value of the best candidate of up to six data sets: nobody (strict comparison)
            planted = [(int(sel[p]), int(np.argmax(Lall[:, sel[p]]))) for p in cs.tie_places(M)]
            thr = base.copy()
            for d, b in planted:
                thr[d] = Lall[b, d]
            got = st.run(thr, params)
            assert got[0] == -1, got[0]
            cs.check_outcome(got, thr, rows, Lall, Lall)
            # one ulp below: the first planted candidate, with exactly the planted fill bits
            thr = base.copy()
            for d, b in planted:
                thr[d] = np.nextafter(Lall[b, d], -np.inf)
            got = st.run(thr, params)
            first = min(b for _, b in planted)
            want = np.zeros(ndata, dtype=bool)
            for d, b in planted:
                want[d] = Lall[first, d] > thr[d]
            assert got[0] == first and np.array_equal(got[1], want[sel]) and got[1].sum() >= 1
            cs.check_outcome(got, thr, rows, Lall, Lall)
            counts["one ulp below"] = (first, int(got[1].sum()))
            # only candidate B - 1 beats anything, and only the first candidate of the last tile of four: that candidate
            # is the own line of spectrum d, every threshold is out of reach but d's, one ulp below it
            for c in cs.lone_candidates(B):
                d, lone = cs.lone_winner(shape, c, params, rows)
                Llone = scorer.loglike_batch(lone)
                assert np.array_equal(np.delete(Llone, c, axis=0), np.delete(Lall, c, axis=0))
                assert cs.strict_margin(Llone, c, d) > 0, "another candidate ties with or beats the planted one"
                thr = np.maximum(base, fs.unbeatable(Llone))
                thr[d] = np.nextafter(Llone[c, d], -np.inf)
                assert fs.decision(Llone, thr, rows)[0] == c and fs.decision(Llone, thr, rows)[1].sum() == 1
                got = st.run(thr, lone)
                assert got[0] == c, (got[0], c)
                cs.check_outcome(got, thr, rows, Llone, Llone)
                assert got[2][d] == Llone[c, d] and got[3].sum() == 1
                counts["lone %d" % c] = (got[0], 1)
        finally:
            names = sorted(st.seen)
            st.close()
            spectra.close()
    print("%s: M = %d, route %s, scored by %s; (accepted, beaten): %s" % (fs.shape_id(shape), M, route or "classic", ", ".join(names), counts))


def _device(spectra):
    return lambda live, shelf_cap: cs.RawDraws(spectra, live, shelf_cap=shelf_cap)


def _show(name, log):
    print("sequence %s: %s" % (name, "; ".join("%s -> %s" % (" x ".join(str(v) for v in entry[:-2]), "%s accepts %d" % (entry[-2] or "classic", entry[-1]))
                                                  for entry in log)))


def test_rows_from_the_mapped_block_then_from_the_device(hip, num_cus):
    """Sequence a: nine chunks and more in ONE draw over a gathered selection (200 spectra, 133 selected, 208 channels,
    shelf_cap = 4).  The first chunk reads the row ids from the mapped block and leaves them on the device, every later
    one reads that copy; the repeated chunks tie with what the shelves hold; fresh faint lines then fill some shelf of
    the selection past the four entries the state was made for: the shelves grow (``room_for_one``) with the selection
    already on the device."""
    x, y = fs.make_inputs(cs.SEQUENCE_A_SHAPE)[:2]
    spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
    try:
        log = cs.sequence_a(LaneScorer(spectra).loglike_batch, _device(spectra), num_cus)
        _show("a", log)
        assert len(log) >= 11
    finally:
        spectra.close()


def test_a_route_switch_inside_a_draw(hip, num_cus):
    """Sequence b: 4097 of 4200 spectra selected (all but every 41st), 8 channels.  Chunks of 8, 9 and 4 candidates:
    two-launch with the rows from the mapped block, classic on the rows that kernel left, two-launch from the device
    copy; a second draw in the order 9, 8, 9: the classic chunk uploads the rows first."""
    x, y, rows = cs.sequence_b_inputs()
    spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
    try:
        log = cs.sequence_b(LaneScorer(spectra).loglike_batch, _device(spectra), num_cus)
        _show("b", log)
        assert len(log) == 6
    finally:
        spectra.close()


def test_both_commit_kernels_on_one_state(hip, num_cus):
    """Sequence c: 300 spectra of 64 channels; draws over selections of 128, 129 and 64 spectra in turn, two chunks
    each: k_chunk_commit, k_joint_commit_trail and k_chunk_commit again on the same shelves and thresholds."""
    x, y = fs.make_inputs((cs.SEQUENCE_C_NDATA, None, cs.SEQUENCE_C_NX, 16))[:2]
    spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
    try:
        log = cs.sequence_c(LaneScorer(spectra).loglike_batch, _device(spectra), num_cus)
        _show("c", log)
        assert len(log) == 6
    finally:
        spectra.close()


def _same(js, ref, what):
    higher, n = js.thresholds()
    assert np.array_equal(n, ref.sizes()), (what, "shelf sizes")
    assert np.array_equal(higher, ref.higher), (what, "thresholds", np.flatnonzero(higher != ref.higher))
    assert np.array_equal(js.shelf_n, n), (what, "the mirror of the sizes")


@pytest.mark.parametrize("shape", cs.HALVES_SHAPES, ids=fs.shape_id)
def test_halves(hip, num_cus, shape):
    """score_backend -> votes / set_votes -> commit_backend on this route, under ordinary thresholds.  The votes of ALL
    candidates (the accept kernel scores every one, so this checks every flag, not only the first); with the first vote
    cleared the second voted candidate is taken in, with its own trail entries; a single foreign vote on a candidate
    nobody accepts is accepted with no bit set and leaves the state as it was; then the honest commit.
    (chunk_support.halves_plan; test_chunk_shapes_host.py: at least two candidates have votes at every shape.)"""
    ndata, _, nx, B = shape
    x, y, params, rows, L_ref = cs.reference(shape)
    M = cs.selection_size(shape)
    route = cs.expected_route(M, B, nx, num_cus)
    spectra = GaussLineSpectra(x, y, noise_level=fs.NOISE)
    js = None
    try:
        Lall = LaneScorer(spectra).loglike_batch(params)
        thr = fs.ordinary_thresholds(L_ref, rows)
        ref, steps = cs.halves_plan(shape, Lall, thr, rows)
        js = cs.backend_state(spectra, cs.NLIVE)
        live = cs.planted_live(thr)
        _lib.check(hip.mdns_joint_set_live(js._h, _lib.ptr(live)), "set_live")
        js.prepare()
        now = cs.Statement(live)
        now.prepare()
        for step, (votes, cast, idx, beats) in enumerate(steps):
            _same(js, now, (step, "before"))
            js.score_backend(params, rows)
            cs.check_route(_kernel(hip), route)
            got = js.votes()
            assert got.dtype == np.int32 and np.array_equal(got, votes), (step, np.flatnonzero(got != votes))
            assert np.array_equal(votes, now.votes(Lall, rows))
            js.set_votes(cast)
            accepted, Lrow, taken = js.commit_backend()
            assert accepted == idx and Lrow is None, (step, accepted, idx)
            assert np.array_equal(taken, beats), (step, np.flatnonzero(taken != beats))
            before = now.higher.copy()
            if beats.any():
                assert np.array_equal(now.commit(Lall, rows, idx), beats)
            _same(js, now, (step, "after"))
            sel = np.arange(ndata) if rows is None else rows
            # (a point that beats its threshold lies above everything waiting: it is the next threshold)
            assert np.array_equal(now.higher[sel[beats]], Lall[idx, sel[beats]])
            assert np.array_equal(now.higher[sel[~beats]], before[sel[~beats]])
        assert np.array_equal(now.higher, ref.higher) and np.array_equal(now.sizes(), ref.sizes())
        print("%s: route %s; votes %s; accepted %s beating %s" % (fs.shape_id(shape), route or "classic", [int(s[0].sum()) for s in steps],
                                                                   [s[2] for s in steps], [int(s[3].sum()) for s in steps]))
    finally:
        if js is not None:
            js.close()
        spectra.close()
