"""The exact K2 row kernels (csrc/mdns_like.hip: k_muse_rows<NP, CB>, k_muse_rows2<NP>, k_muse_rows_generic) at the
edges of their channel blocks and of their three launch shapes: against the longdouble statement, and for what a
template row may read -- its own ``model_ld(nx)`` doubles and nothing of the next row or of the scratch behind the last.

Every launch is followed by a look at ``mdns_profile_kernel(1)``: a case that takes another instantiation than the one
it was built for fails instead of passing vacuously.  The tests of what a row reads detect an over-read by VALUE, inside
memory the library owns: each of them first makes a larger call on the handle, so that the block behind the templates
is allocated and holds what the test put there."""
import os
import sys

import numpy as np
import pytest

from massivedatans_amd import _lib, gen, jointstate, musefuse
from massivedatans_amd.like import MuseSpectra
import k2_rows_support as ks
from k2_rows_support import RTOL_L, RTOL_SLOT, case, rel_err, selection, statement

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def num_cus():
    """``torch.cuda.get_device_properties(0).multi_processor_count``, asked in a child process: torch brings a HIP
    runtime of its own and finds no device in a process where the library's runtime came first -- which is every run of
    the whole suite in one process."""
    import subprocess
    code = "import torch; print(int(torch.cuda.get_device_properties(0).multi_processor_count))"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.strip().splitlines()[-1])


def launched():
    return (_lib.load().mdns_profile_kernel(1) or b"").decode()


def score(sp, ypred, rows, num_cus):
    """``loglike_batch`` plus the check of which kernel ran."""
    got = sp.loglike_batch(ypred, rows)
    M = sp.ndata if rows is None else len(rows)
    assert launched() == ks.expected_kernel(sp.nx, len(ypred), M, num_cus), (launched(), sp.nx, len(ypred), M)
    return got


def spectra_of(d, **kw):
    return MuseSpectra(d["x"], d["y"], d["v"], **kw)


# ------------------------------------------------------------------ (a) the statement, at every block edge
# both edges of every NP (1 | 512, 513 | 1024, 1025 | 1536, ... 3585 | 4096), values inside, and the generic kernel behind
SWEEP_NX = [3, 7, 255, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 2560, 2561, 3072, 3073,
            3583, 3584, 3585, 4095, 4096, 4097, 4610]


@pytest.mark.parametrize("nx", SWEEP_NX)
def test_rows_against_the_statement(nx, num_cus):
    """Every nx under all three launch shapes: one candidate (B = 1), pairs of candidates (B = 2, 5, 33 on 1, 3 and 70
    spectra: the odd counts end on a clamped partner, the few spectra split the candidates over grid.y) and two spectra
    per workgroup (B = 5 on 2 num_cus + 1 spectra: the last workgroup's second row is the clamped one); all spectra, a
    sparse odd selection with the last row, and ids in no order with repeats.  1e-11 against the longdouble statement,
    computed once per cube."""
    many = 2 * num_cus + 1
    worst = 0.0
    for ndata, Bs in ((1, (1, 2, 33)), (3, (1, 5, 33)), (70, (1, 2, 5)), (many, (5,))):
        d = case(nx, ndata, max(Bs))
        want = statement(d["y"], d["v"], d["ypred"])
        sp = spectra_of(d)
        rng = np.random.RandomState(nx + ndata)
        for B in Bs:
            for rows in (None, selection(ndata, True, rng), ks.scrambled(ndata, rng)):
                got = score(sp, d["ypred"][:B], rows, num_cus)
                if ndata == many and nx <= 4096 and (rows is None or len(rows) == many):
                    assert launched().startswith("k_muse_rows2<"), launched()
                ref = want[:B] if rows is None else want[:B][:, rows]
                assert got.shape == ref.shape
                err = rel_err(got, ref)
                worst = max(worst, err)
                assert err < RTOL_L, (nx, ndata, B, launched(), err)
        sp.close()
    print("nx=%d: max rel err %.3g against the longdouble statement" % (nx, worst))


@pytest.mark.parametrize("nx", [1, 2])
def test_near_perfect_fits_in_absolute_terms(nx, num_cus):
    """One and two channels: the scale fits (almost) everything, chi -> 0, and the float64 statement itself is off by 100 %
    (nx = 1) and 5e-12 (nx = 2) in relative terms.  In absolute terms: within 1e-11 of the size of the sum it is what is
    left of, 0.5 sum y^2 w, per spectrum."""
    for ndata, B in ((3, 2), (70, 1), (2 * num_cus + 1, 5)):
        d = case(nx, ndata, B)
        want = statement(d["y"], d["v"], d["ypred"])
        size = 0.5 * (np.asarray(d["y"], dtype=np.longdouble) ** 2 / np.asarray(d["v"], dtype=np.longdouble)).sum(axis=0)
        sp = spectra_of(d)
        got = score(sp, d["ypred"], None, num_cus)
        dev = np.abs(got.astype(np.longdouble) - want) / size[None, :]
        print("nx=%d ndata=%d B=%d %s: max |got - want| / (0.5 sum y^2 w) %.3g" % (nx, ndata, B, launched(), float(dev.max())))
        assert np.all(dev <= 1e-11)
        sp.close()


# ------------------------------------------------------------------ (b) a template is scored by itself
# [good, NaN, good, good, +inf, good, good]: a bad row directly behind a good one (0 -> 1, 3 -> 4) and one two rows behind
# (2 -> 4: what eight channel blocks on rows of five or six reach)
BAD = {1: np.nan, 4: np.inf}
GOOD = [0, 2, 3, 5, 6]


def _with_bad(templates):
    out = templates.copy()
    for b, value in BAD.items():
        out[b] = value
    return out


def _isolation(sp, templates, rows, num_cus):
    """Scores ``templates`` with the rows of BAD made non-finite and as they are; the good candidates must not notice."""
    clean = score(sp, templates, rows, num_cus)
    dirty = score(sp, _with_bad(templates), rows, num_cus)
    assert np.isfinite(clean).all()
    for b in BAD:
        assert not np.isfinite(dirty[b]).any(), b
    for b in GOOD:
        assert np.array_equal(dirty[b], clean[b]), ("candidate %d read another candidate's template" % b, launched())


@pytest.mark.parametrize("nx", [1024, 1025, 1536, 2048, 2049, 3072, 3584, 4096])
@pytest.mark.parametrize("shape", ["one", "pairs", "two_rows"])
def test_a_template_is_scored_by_itself(nx, shape, num_cus):
    """A candidate whose template is not finite gets a non-finite likelihood, for every spectrum, and nobody else does: the
    good candidates' rows are, bit for bit, what they are with finite templates in the bad ones' places (same B, M and
    instantiation).  ``one``: a launch scores one candidate, so the bad template is what the call before left in the
    next row."""
    ndata = {"one": 3, "pairs": 3, "two_rows": 2 * num_cus + 1}[shape]
    d = case(nx, ndata, 9)
    sp = spectra_of(d)
    score(sp, d["ypred"], None, num_cus)                        # nine rows of scratch, all finite
    if shape == "one":
        clean = score(sp, d["ypred"][:1], None, num_cus)
        three = score(sp, np.vstack((d["ypred"][:1], np.full((2, nx), np.nan))), None, num_cus)
        assert not np.isfinite(three[1:]).any()
        after = score(sp, d["ypred"][:1], None, num_cus)        # rows 1 and 2 of the scratch still hold the NaN
        assert np.isfinite(clean).all() and np.array_equal(after, clean), "the candidate read the row behind its own"
    else:
        assert ks.variant(7, ndata, num_cus) == (1 if shape == "pairs" else 2)
        _isolation(sp, d["ypred"][:7], None, num_cus)
        if shape == "pairs":
            _isolation(sp, d["ypred"][:7], np.array([2, 0, 2], dtype=np.int32), num_cus)
    sp.close()


def test_a_template_is_scored_by_itself_with_a_continuum():
    """The same through k_continuum_rows, which tests its template load: 1100 channels in four channel blocks."""
    from continuum_support import case as continuum_case
    d = continuum_case(1100, 3, 1, 9)
    sp = spectra_of(d, continuum=1)
    sp.loglike_batch(d["ypred"])
    clean = sp.loglike_batch(d["ypred"][:7])
    dirty = sp.loglike_batch(_with_bad(d["ypred"][:7]))
    assert launched() == "k_continuum_rows<4, 1>", launched()
    assert np.isfinite(clean).all()
    for b in BAD:
        assert not np.isfinite(dirty[b]).any()
    for b in GOOD:
        assert np.array_equal(dirty[b], clean[b]), b
    sp.close()


# ------------------------------------------------------------------ (c) stale scratch behind the last row
@pytest.mark.parametrize("nx", [1100, 2050, 3000])
@pytest.mark.parametrize("B,shape", [(1, "one"), (2, "pairs"), (5, "pairs"), (5, "two_rows")])
def test_stale_scratch_behind_the_last_row(nx, B, shape, num_cus):
    """The scratch of a handle only grows: after a batch of B + 2 templates whose last two are NaN, a batch of B finite
    ones ends right in front of them.  Its likelihoods are finite and equal, bit for bit, those of the same call on a
    fresh handle (whose scratch a batch of B + 2 finite templates made as large)."""
    ndata = 2 * num_cus + 1 if shape == "two_rows" else 3
    d = case(nx, ndata, B + 2)
    assert ks.variant(B, ndata, num_cus) == {"one": 0, "pairs": 1, "two_rows": 2}[shape]
    used, fresh = spectra_of(d), spectra_of(d)
    poison = d["ypred"].copy()
    poison[B:] = np.nan
    assert not np.isfinite(score(used, poison, None, num_cus)[B:]).any()
    got = score(used, d["ypred"][:B], None, num_cus)
    score(fresh, d["ypred"][::-1].copy(), None, num_cus)
    want = score(fresh, d["ypred"][:B], None, num_cus)
    assert np.isfinite(want).all()
    assert np.isfinite(got).all(), "the last candidate read the scratch behind its row"
    assert np.array_equal(got, want)
    used.close()
    fresh.close()


def test_stale_scratch_behind_a_committed_row_of_the_filter(num_cus):
    """The same on templates ``model_ld(nx) + 16`` apart: a chunk of two that the matrix-core filter settled is committed
    through the exact kernel (mdns_backend_draw_band_commit), after a chunk of six whose third candidate was NaN -- which
    is what lies behind the second row of the small chunk.  The committed row, read back from the live matrix, equals
    bit for bit what the exact kernel gives for that pair on a handle of its own, and fills what it must."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k2_filter_bench as kb
    nx, ndata, nlive = 1100, 40, 8
    rng = np.random.RandomState(1100)
    cube = gen.muse_like(ndata, nx)
    lib = _lib.load()
    sp, other = MuseSpectra(cube["x"], cube["y"], cube["v"]), MuseSpectra(cube["x"], cube["y"], cube["v"])
    js = jointstate.MuseJointState(sp, nlive, shelf_cap=4)
    try:
        js.init(musefuse.priortransform_batch(rng.uniform(size=(nlive, 5))))
        arg = js.prepare()[1]
        Lmin = js.thresholds()[0]
        six = musefuse.priortransform_batch(rng.uniform(size=(6, 5)))
        # the truth of spectra 0 and 1: each beats every live point of its spectrum, and nothing comes near a threshold
        two = np.array([(0.0, cube["z"][0], 0.0, 1.0, 1.0), (0.0, cube["z"][1], 0.0, 1.0, 1.0)])
        other.loglike_batch_lines(six)                               # (the reference's own scratch: six finite rows)
        exact = other.loglike_batch_lines(two)
        assert launched() == ks.expected_kernel(nx, 2, ndata, num_cus)
        beats = exact[1] > Lmin
        assert beats[1] and np.min(np.abs(exact - Lmin) / np.abs(Lmin)) > 1e-6
        six[2, 0] = np.nan
        assert np.isnan(other.templates(six)[2]).all()
        bound = np.full(6, 1e-9)
        kb.band(js, six, None, bound, 1)
        status, npairs = kb.band(js, two, None, bound[:2], 1)[:2]
        assert npairs == 0 and status[1] == 1, (status, npairs)
        assert launched().startswith("k_muse_gemm_band"), launched()          # (nothing scored the chunk again exactly)
        bits, no_noise = np.zeros((ndata + 63) // 64, dtype=np.uint64), np.zeros(ndata)
        js._check(lib.mdns_backend_draw_band_commit(js._h, 1, _lib.ptr(no_noise), _lib.ptr(bits)), "mdns_backend_draw_band_commit")
        assert launched() == ks.expected_kernel(nx, 2, ndata, num_cus), launched()
        got = np.unpackbits(bits.view(np.uint8), bitorder='little')[:ndata].astype(bool)
        assert np.array_equal(got, beats)
        js.took(None, got)
        k = np.flatnonzero(beats).astype(np.int32)                   # the spectra that have a point waiting: one iteration of those
        js.set_running(k)
        js.prepare()
        js.advance()
        after = js.live_matrix()
        assert after.shape == (nlive, len(k))
        assert np.array_equal(after[arg[k], np.arange(len(k))], exact[1, k])
    finally:
        lib.mdns_muse_filter_mode(-1)
        js.close()
        sp.close()
        other.close()


# ------------------------------------------------------------------ (d) one value per pair
def _same_parity_permutation(B, rng):
    perm = np.arange(B)
    perm[0::2] = rng.permutation(perm[0::2])
    perm[1::2] = rng.permutation(perm[1::2])
    return perm


@pytest.mark.parametrize("nx", [1100, 3000, 4096])
def test_a_pair_has_one_value(nx, num_cus):
    """The bits of L for (template b, spectrum k) depend on the instantiation and, where candidates go in pairs, on the
    candidate's place in its pair (muse_rows_variant) -- and, where spectra go in twos (k_muse_rows2), on the spectrum's
    place in its two, for the same reason: the four sums of a workgroup go through one permlane-swap reduction whose
    four results associate differently.  On nothing else: not on M, the selection, the other candidates of the launch or
    the split of the candidates over grid.y.  Across instantiations and places: 1e-13."""
    rng = np.random.RandomState(nx)
    d = case(nx, 70, 33)
    t = d["ypred"]
    sp = spectra_of(d)
    whole = score(sp, t, None, num_cus)                                        # pairs, split over grid.y
    for k in (0, 69, 33):
        assert np.array_equal(score(sp, t, np.array([k], dtype=np.int32), num_cus)[:, 0], whole[:, k])          # M = 1 against M = 70
    sel = selection(70, True, rng)
    assert np.array_equal(score(sp, t, sel, num_cus), whole[:, sel])
    mixed = ks.scrambled(70, rng)
    assert np.array_equal(score(sp, t, mixed, num_cus), whole[:, mixed])
    perm = _same_parity_permutation(33, rng)                                   # other neighbours, the same place in the pair
    assert np.array_equal(score(sp, t[perm], sel, num_cus), whole[perm][:, sel])
    assert np.array_equal(score(sp, t[4:10], None, num_cus), whole[4:10])      # another launch, another split
    assert np.array_equal(score(sp, t[[32, 5]], None, num_cus), whole[[32, 5]])  # 32: its partner was itself, now it is 5
    swapped = score(sp, t[[5, 32]], None, num_cus)                             # the other place in the pair
    assert rel_err(swapped, whole[[5, 32]]) < RTOL_SLOT
    for b in (0, 17, 32):                                                      # one candidate per launch: another instantiation
        alone = score(sp, t[b:b + 1], None, num_cus)
        assert launched().endswith(", 1>") and rel_err(alone, whole[b:b + 1]) < RTOL_SLOT
    sp.close()
    # 33 candidates on 3 spectra (split over grid.y, odd tail) against the same templates scored two at a time
    d3 = case(nx, 3, 33)
    sp = spectra_of(d3)
    whole = score(sp, d3["ypred"], None, num_cus)
    for b in range(0, 32, 2):
        assert np.array_equal(score(sp, d3["ypred"][b:b + 2], None, num_cus), whole[b:b + 2]), b
    # (the odd one out would go alone through <NP, 1>: with a partner instead, and in the first place as in the 33)
    assert np.array_equal(score(sp, d3["ypred"][[32, 0]], None, num_cus)[0], whole[32])
    assert rel_err(score(sp, d3["ypred"][32:], None, num_cus), whole[32:]) < RTOL_SLOT
    sp.close()
    # two spectra per workgroup
    many = 2 * num_cus + 1
    dm = case(nx, many, 5)
    sp = spectra_of(dm)
    whole = score(sp, dm["ypred"], None, num_cus)
    assert launched().startswith("k_muse_rows2<")
    perm = _same_parity_permutation(many, rng).astype(np.int32)                # other neighbours, the same place in the two
    assert np.array_equal(score(sp, dm["ypred"], perm, num_cus), whole[:, perm])
    assert np.array_equal(score(sp, dm["ypred"][[3, 0, 4, 1]], None, num_cus), whole[[3, 0, 4, 1]])   # any candidates, any order
    shifted = np.roll(np.arange(many), 1).astype(np.int32)                     # the other place in the two
    assert rel_err(score(sp, dm["ypred"], shifted, num_cus), whole[:, shifted]) < RTOL_SLOT
    few = selection(many, True, rng)                                           # pairs of candidates: another instantiation
    assert rel_err(score(sp, dm["ypred"], few, num_cus), whole[:, few]) < RTOL_SLOT and launched().endswith(", 2>")
    sp.close()


# ------------------------------------------------------------------ (e) rows looped inside a workgroup
@pytest.mark.parametrize("B", [2, 5])
def test_rows_looped_inside_a_workgroup(B, num_cus):
    """More spectra than the grid has workgroups (8 num_cus): 37 of them are a workgroup's second trip, and for two
    spectra per workgroup the last two are half empty.  The output buffer is poisoned first: every entry must be written,
    and equal the statement."""
    nx, ndata = 8, 8 * num_cus + 37
    d = case(nx, ndata, B)
    want = statement(d["y"], d["v"], d["ypred"])
    sp = spectra_of(d)
    lib = _lib.load()
    got = np.full((B, ndata), np.nan)
    templates = np.ascontiguousarray(d["ypred"])
    d_L, d_t = lib.mdns_dev_alloc(got.nbytes), lib.mdns_dev_alloc(templates.nbytes)
    try:
        assert d_L and d_t
        _lib.check(lib.mdns_h2d(d_L, _lib.ptr(got), got.nbytes), "mdns_h2d")          # poison
        _lib.check(lib.mdns_h2d(d_t, _lib.ptr(templates), templates.nbytes), "mdns_h2d")
        _lib.check(lib.mdns_muse_loglike_batch_dev(sp.handle, d_t, B, None, ndata, d_L), "mdns_muse_loglike_batch_dev")
        _lib.check(lib.mdns_d2h(_lib.ptr(got), d_L, got.nbytes), "mdns_d2h")
    finally:
        for p in (d_L, d_t):
            if p:
                lib.mdns_dev_free(p)
    assert launched() == ks.expected_kernel(nx, B, ndata, num_cus) == ("k_muse_rows<1, 2>" if B == 2 else "k_muse_rows2<1>")
    assert np.isfinite(got).all(), "entries left untouched: %d" % (~np.isfinite(got)).sum()
    err = rel_err(got, want)
    print("B=%d ndata=%d %s: max rel err %.3g" % (B, ndata, launched(), err))
    assert err < RTOL_L
    sp.close()


# ------------------------------------------------------------------ (f) the other doors to the same launch
def test_templates_made_on_the_device_are_scored_by_themselves(num_cus):
    """loglike_batch_lines at nx = 1100: three candidates, the middle one with a NaN parameter and so a NaN template."""
    d = case(1100, 5, 5)
    sp = spectra_of(d)
    sp.loglike_batch_lines(d["params"])                              # five rows of scratch, all finite
    params = d["params"][:3].copy()
    clean = sp.loglike_batch_lines(params)
    assert launched() == ks.expected_kernel(1100, 3, 5, num_cus)
    templates = sp.templates(params)
    params[1, 0] = np.nan
    assert np.isnan(sp.templates(params)[1]).all()
    dirty = sp.loglike_batch_lines(params)
    assert launched() == ks.expected_kernel(1100, 3, 5, num_cus)
    assert not np.isfinite(dirty[1]).any()
    assert np.array_equal(dirty[[0, 2]], clean[[0, 2]])
    assert rel_err(clean, statement(d["y"], d["v"], templates)) < RTOL_L
    sp.close()


def test_curves_of_a_joint_state_are_scored_by_themselves(num_cus):
    """The scale-marginalised curve route (mdns_joint_init_curves on spectra with variances): three live points, the
    middle one's curve NaN."""
    d = case(1100, 5, 5)
    sp = spectra_of(d)
    score(sp, d["ypred"], None, num_cus)                             # five rows of scratch, all finite
    curves = d["ypred"][:3].copy()
    out = []
    for bad in (False, True):
        if bad:
            curves[1] = np.nan
        js = jointstate.CurveJointState(sp, 3, lambda xs: curves[np.asarray(xs[:, 0], dtype=int)], ndim=1)
        js.init(np.arange(3.0)[:, None])
        assert launched() == ks.expected_kernel(1100, 3, 5, num_cus)
        out.append(js.live_matrix())
        js.close()
    clean, dirty = out
    assert not np.isfinite(dirty[1]).any()
    assert np.array_equal(dirty[[0, 2]], clean[[0, 2]])
    assert rel_err(clean, statement(d["y"], d["v"], d["ypred"][:3])) < RTOL_L
    sp.close()


def test_the_drop_in_scores_its_template_by_itself(hip, num_cus):
    """mdns_muse_like on registered spectra (one handle for all calls, one template per call) with a partial mask: a NaN
    template gives NaN where the mask is set and nothing elsewhere; the finite template after it is not touched by what
    the call before left in the scratch, and gives what the statement and a handle of its own give.  (This door scores
    one template per call into row 0 of its handle's scratch, so the words behind that row are never written through it:
    a kernel that read them would see what the allocation happened to hold, and this case alone may miss it.)"""
    nx, nd = 1100, 6
    d = case(nx, nd, 2)
    y, v = np.ascontiguousarray(d["y"]), np.ascontiguousarray(d["v"])
    mask = np.array([True, False, True, True, False, True])
    M = int(mask.sum())
    good = np.ascontiguousarray(d["ypred"][0])
    own = spectra_of(d)
    score(own, d["ypred"], None, num_cus)
    want_bits = score(own, d["ypred"][:1], mask, num_cus)[0]
    own.close()
    assert hip.mdns_register_spectra(_lib.ptr(y), _lib.ptr(v), nd, nx) == 0
    try:
        for template, finite in ((np.full(nx, np.nan), False), (good, True)):
            L = np.full(nd, 12345.0)
            assert hip.mdns_muse_like(_lib.ptr(y), _lib.ptr(v), _lib.ptr(template), _lib.ptr(mask), nd, nx, _lib.ptr(L)) == 0, _lib.last_error()
            assert launched() == ks.expected_kernel(nx, 1, M, num_cus)
            assert np.all(L[~mask] == 12345.0)
            assert np.isfinite(L[mask]).all() if finite else np.isnan(L[mask]).all()
        assert np.array_equal(L[mask], want_bits)
        assert rel_err(L[mask], statement(y, v, good, np.flatnonzero(mask))[0]) < RTOL_L
    finally:
        assert hip.mdns_unregister_spectra(_lib.ptr(y)) == 0
