"""What the joint state's parameter-taking entry points refuse, and in which words (csrc/mdns_joint.hip): one joint state
per statistic -- fixed noise, scale-marginalised, fixed scale, Poisson, W statistic --, every entry on each with otherwise
valid arguments, and the backend entries once more without a draw begun.  Every cell is either served or refused with
exactly the text of EXPECTED; a refused call leaves ``*accepted == -1`` where the entry has that output and the state
usable (a curve chunk right behind it succeeds).  Every refusal is taken on the host, before anything is launched.

EXPECTED was recorded from this file's ``observe`` on the commit BEFORE the entry preamble and the model tag were
folded into one function each: it pins the texts and, where an entry refuses for two reasons, which one it names."""
import ctypes as C

import numpy as np
import pytest

from massivedatans_amd import _lib, jointstate
from massivedatans_amd.like import CountSpectra, GaussLineSpectra, MuseSpectra, WeightedSpectra

pytestmark = pytest.mark.gpu

NDATA, NX, NLIVE, B = 3, 8, 4, 2
STATES = ("gauss", "muse", "chi2", "poisson", "wstat")

_ONLY = " spectra take curve chunks only (mdns_joint_init_curves, mdns_backend_draw_curves)"

# (state, entry, a draw begun?) -> None: served; or the text of mdns_last_error()
EXPECTED = {
    ('gauss', 'mdns_joint_init_gauss', True): None,
    ('gauss', 'mdns_joint_init_muse3', True): 'mdns_joint_init_muse3: the spectra carry no variances',
    ('gauss', 'mdns_joint_score_dev', True): None,
    ('gauss', 'mdns_backend_draw_chunk', True): None,
    ('gauss', 'mdns_backend_draw_score', True): None,
    ('gauss', 'mdns_backend_draw_band_begin', True): 'mdns_backend_draw_band: a state of the scale-marginalised likelihood is needed',
    ('gauss', 'mdns_backend_draw_band', True): 'mdns_backend_draw_band: a state of the scale-marginalised likelihood is needed',
    ('gauss', 'mdns_backend_draw_band_commit', True): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('muse', 'mdns_joint_init_gauss', True): 'mdns_joint_init_gauss: these spectra carry variances (mdns_joint_init_muse3)',
    ('muse', 'mdns_joint_init_muse3', True): None,
    ('muse', 'mdns_joint_score_dev', True): 'mdns_joint_score_dev: Gaussian-line states only (use the mdns_backend_* entry points)',
    ('muse', 'mdns_backend_draw_chunk', True): None,
    ('muse', 'mdns_backend_draw_score', True): None,
    ('muse', 'mdns_backend_draw_band_begin', True): None,
    ('muse', 'mdns_backend_draw_band', True): None,
    ('muse', 'mdns_backend_draw_band_commit', True): None,
    ('chi2', 'mdns_joint_init_gauss', True): 'mdns_joint_init_gauss: fixed-scale' + _ONLY,
    ('chi2', 'mdns_joint_init_muse3', True): 'mdns_joint_init_muse3: fixed-scale' + _ONLY,
    ('chi2', 'mdns_joint_score_dev', True): 'mdns_joint_score_dev: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_chunk', True): 'mdns_backend_draw_chunk: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_score', True): 'mdns_backend_draw_score: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_band_begin', True): 'mdns_backend_draw_band: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_band', True): 'mdns_backend_draw_band: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_band_commit', True): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('poisson', 'mdns_joint_init_gauss', True): 'mdns_joint_init_gauss: counts' + _ONLY,
    ('poisson', 'mdns_joint_init_muse3', True): 'mdns_joint_init_muse3: counts' + _ONLY,
    ('poisson', 'mdns_joint_score_dev', True): 'mdns_joint_score_dev: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_chunk', True): 'mdns_backend_draw_chunk: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_score', True): 'mdns_backend_draw_score: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_band_begin', True): 'mdns_backend_draw_band: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_band', True): 'mdns_backend_draw_band: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_band_commit', True): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('wstat', 'mdns_joint_init_gauss', True): 'mdns_joint_init_gauss: counts' + _ONLY,
    ('wstat', 'mdns_joint_init_muse3', True): 'mdns_joint_init_muse3: counts' + _ONLY,
    ('wstat', 'mdns_joint_score_dev', True): 'mdns_joint_score_dev: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_chunk', True): 'mdns_backend_draw_chunk: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_score', True): 'mdns_backend_draw_score: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_band_begin', True): 'mdns_backend_draw_band: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_band', True): 'mdns_backend_draw_band: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_band_commit', True): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('gauss', 'mdns_backend_draw_chunk', False): 'mdns_backend_draw_chunk: no draw begun',
    ('gauss', 'mdns_backend_draw_score', False): 'mdns_backend_draw_score: no draw begun',
    ('gauss', 'mdns_backend_draw_band_begin', False): 'mdns_backend_draw_band: a state of the scale-marginalised likelihood is needed',
    ('gauss', 'mdns_backend_draw_band', False): 'mdns_backend_draw_band: a state of the scale-marginalised likelihood is needed',
    ('gauss', 'mdns_backend_draw_band_commit', False): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('gauss', 'mdns_backend_draw_curves', False): 'mdns_backend_draw_curves: no draw begun',
    ('gauss', 'mdns_backend_draw_curves_dev', False): 'mdns_backend_draw_curves_dev: no draw begun',
    ('gauss', 'mdns_backend_draw_table', False): 'mdns_backend_draw_table: null table handle',
    ('muse', 'mdns_backend_draw_chunk', False): 'mdns_backend_draw_chunk: no draw begun',
    ('muse', 'mdns_backend_draw_score', False): 'mdns_backend_draw_score: no draw begun',
    ('muse', 'mdns_backend_draw_band_begin', False): 'mdns_backend_draw_band: no draw begun',
    ('muse', 'mdns_backend_draw_band', False): 'mdns_backend_draw_band: no draw begun',
    ('muse', 'mdns_backend_draw_band_commit', False): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('muse', 'mdns_backend_draw_curves', False): 'mdns_backend_draw_curves: no draw begun',
    ('muse', 'mdns_backend_draw_curves_dev', False): 'mdns_backend_draw_curves_dev: no draw begun',
    ('muse', 'mdns_backend_draw_table', False): 'mdns_backend_draw_table: null table handle',
    ('chi2', 'mdns_backend_draw_chunk', False): 'mdns_backend_draw_chunk: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_score', False): 'mdns_backend_draw_score: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_band_begin', False): 'mdns_backend_draw_band: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_band', False): 'mdns_backend_draw_band: fixed-scale' + _ONLY,
    ('chi2', 'mdns_backend_draw_band_commit', False): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('chi2', 'mdns_backend_draw_curves', False): 'mdns_backend_draw_curves: no draw begun',
    ('chi2', 'mdns_backend_draw_curves_dev', False): 'mdns_backend_draw_curves_dev: no draw begun',
    ('chi2', 'mdns_backend_draw_table', False): 'mdns_backend_draw_table: null table handle',
    ('poisson', 'mdns_backend_draw_chunk', False): 'mdns_backend_draw_chunk: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_score', False): 'mdns_backend_draw_score: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_band_begin', False): 'mdns_backend_draw_band: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_band', False): 'mdns_backend_draw_band: counts' + _ONLY,
    ('poisson', 'mdns_backend_draw_band_commit', False): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('poisson', 'mdns_backend_draw_curves', False): 'mdns_backend_draw_curves: no draw begun',
    ('poisson', 'mdns_backend_draw_curves_dev', False): 'mdns_backend_draw_curves_dev: no draw begun',
    ('poisson', 'mdns_backend_draw_table', False): 'mdns_backend_draw_table: null table handle',
    ('wstat', 'mdns_backend_draw_chunk', False): 'mdns_backend_draw_chunk: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_score', False): 'mdns_backend_draw_score: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_band_begin', False): 'mdns_backend_draw_band: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_band', False): 'mdns_backend_draw_band: counts' + _ONLY,
    ('wstat', 'mdns_backend_draw_band_commit', False): 'mdns_backend_draw_band_commit: candidate 0 of a chunk of 0',
    ('wstat', 'mdns_backend_draw_curves', False): 'mdns_backend_draw_curves: no draw begun',
    ('wstat', 'mdns_backend_draw_curves_dev', False): 'mdns_backend_draw_curves_dev: no draw begun',
    ('wstat', 'mdns_backend_draw_table', False): 'mdns_backend_draw_table: null table handle',
}


def _spectra(kind):
    rng = np.random.RandomState(5)
    x = np.linspace(4750.0, 9350.0, NX)
    y = 1.0 + 0.1 * rng.normal(size=(NX, NDATA))
    v = rng.uniform(0.5, 2.0, size=(NX, NDATA)) * 1e-2
    n = rng.poisson(5.0, size=(NX, NDATA)).astype(float)
    if kind == "gauss":
        return GaussLineSpectra(x, y, noise_level=0.1)
    if kind == "muse":
        return MuseSpectra(x, y, v)
    if kind == "chi2":
        return WeightedSpectra(x, y, v)
    if kind == "poisson":
        return CountSpectra(x, n)
    return CountSpectra(x, n, background=rng.poisson(2.0, size=(NX, NDATA)).astype(float))


class _Args(object):
    """Valid arguments for every entry, kept alive for the whole module."""

    def __init__(self, lib):
        rng = np.random.RandomState(6)
        self.lib = lib
        self.gauss = np.ascontiguousarray(np.column_stack([np.full(NLIVE, 1.0), np.linspace(5000, 9000, NLIVE), np.full(NLIVE, 800.0)]))
        self.muse = np.ascontiguousarray(np.column_stack([np.full(NLIVE, -3.0), rng.uniform(0, 0.02, NLIVE), rng.uniform(-0.5, 0.5, NLIVE),
                                                          np.ones(NLIVE), np.ones(NLIVE)]))
        self.live_curves = np.ascontiguousarray(1.0 + 0.05 * rng.uniform(size=(NLIVE, NX)))
        self.curves = np.ascontiguousarray(1.0 + 0.05 * rng.uniform(size=(B, NX)))
        self.bound = np.zeros(B)
        self.row = np.zeros(NDATA)
        self.bits = np.zeros(1, dtype=np.uint64)
        self.accepted, self.nscored, self.npairs = C.c_int(7), C.c_int(0), C.c_int(0)
        self.status = np.zeros(B, dtype=np.int32)
        self.pb, self.pk = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32)
        self.pL, self.pt = np.zeros(64), np.zeros(64)
        self.d_gauss = lib.mdns_dev_alloc(self.gauss.nbytes)
        self.d_curves = lib.mdns_dev_alloc(self.curves.nbytes)
        assert self.d_gauss and self.d_curves
        _lib.check(lib.mdns_h2d(self.d_gauss, _lib.ptr(self.gauss), self.gauss.nbytes), "mdns_h2d")
        _lib.check(lib.mdns_h2d(self.d_curves, _lib.ptr(self.curves), self.curves.nbytes), "mdns_h2d")

    def close(self):
        self.lib.mdns_dev_free(self.d_gauss)
        self.lib.mdns_dev_free(self.d_curves)

    def params(self, spectra):
        """Parameter rows of the width a state on ``spectra`` takes, if it takes any: 3 of the Gaussian line, else 5."""
        return self.gauss if isinstance(spectra, GaussLineSpectra) else self.muse

    def out(self):
        self.accepted.value = 7
        return C.addressof(self.accepted), _lib.ptr(self.bits), C.addressof(self.nscored)

    def band_out(self):
        return (_lib.ptr(self.status), C.addressof(self.npairs), _lib.ptr(self.pb), _lib.ptr(self.pk), _lib.ptr(self.pL), _lib.ptr(self.pt), 64)


# every entry: f(lib, a, st) -> (rc, has the entry an *accepted?); what a served call leaves in flight is collected
def _init_gauss(lib, a, st):
    return lib.mdns_joint_init_gauss(st._h, _lib.ptr(a.gauss), 0.1), False


def _init_muse3(lib, a, st):
    return lib.mdns_joint_init_muse3(st._h, _lib.ptr(a.muse), None), False


def _score_dev(lib, a, st):
    rc = lib.mdns_joint_score_dev(st._h, a.d_gauss, B, 0.1, None, NDATA)
    if rc == 0:
        assert lib.mdns_joint_commit_bits_dev(st._h, None, NDATA) == 0
        assert lib.mdns_joint_fetch(st._h, NDATA, C.addressof(a.accepted), _lib.ptr(a.bits)) == 0
    return rc, False


def _draw_chunk(lib, a, st):
    return lib.mdns_backend_draw_chunk(st._h, _lib.ptr(a.params(st.spectra)), B, None, *a.out()), True


def _draw_score(lib, a, st):
    rc = lib.mdns_backend_draw_score(st._h, _lib.ptr(a.params(st.spectra)), B, None)
    if rc == 0:
        assert lib.mdns_backend_draw_commit(st._h, C.addressof(a.accepted), _lib.ptr(a.bits)) == 0
    return rc, False


def _band_begin(lib, a, st):
    rc = lib.mdns_backend_draw_band_begin(st._h, _lib.ptr(a.params(st.spectra)), B, _lib.ptr(a.bound))
    if rc == 0:
        assert lib.mdns_backend_draw_band_end(st._h, *a.band_out()) == 0
    return rc, False


def _band(lib, a, st):
    return lib.mdns_backend_draw_band(st._h, _lib.ptr(a.params(st.spectra)), B, _lib.ptr(a.bound), *a.band_out()), False


def _band_commit(lib, a, st):
    _band(lib, a, st)                                   # (the chunk a commit belongs to, where the state serves one)
    return lib.mdns_backend_draw_band_commit(st._h, 0, _lib.ptr(a.row), _lib.ptr(a.bits)), False


def _draw_curves(lib, a, st):
    return lib.mdns_backend_draw_curves(st._h, _lib.ptr(a.curves), B, None, *a.out()), True


def _draw_curves_dev(lib, a, st):
    return lib.mdns_backend_draw_curves_dev(st._h, a.d_curves, NX, B, None, *a.out()), True


def _draw_table_null(lib, a, st):
    return lib.mdns_backend_draw_table(st._h, None, _lib.ptr(a.gauss), B, None, *a.out()), True


PARAMETER_ENTRIES = (("mdns_joint_init_gauss", _init_gauss), ("mdns_joint_init_muse3", _init_muse3), ("mdns_joint_score_dev", _score_dev),
                     ("mdns_backend_draw_chunk", _draw_chunk), ("mdns_backend_draw_score", _draw_score),
                     ("mdns_backend_draw_band_begin", _band_begin), ("mdns_backend_draw_band", _band),
                     ("mdns_backend_draw_band_commit", _band_commit))
BACKEND_ENTRIES = PARAMETER_ENTRIES[3:] + (("mdns_backend_draw_curves", _draw_curves), ("mdns_backend_draw_curves_dev", _draw_curves_dev),
                                           ("mdns_backend_draw_table", _draw_table_null))
CELLS = [(s, name, True, f) for s in STATES for name, f in PARAMETER_ENTRIES] + \
        [(s, name, False, f) for s in STATES for name, f in BACKEND_ENTRIES]


def _curve_chunk(lib, a, st):
    """A valid curve chunk over every data set, from its draw_begin on."""
    return lib.mdns_backend_draw_begin(st._h, None, NDATA) == 0 and _draw_curves(lib, a, st)[0] == 0


def observe():
    """{(state, entry, begun): (error text or None, *accepted after a refusal or None, usable after a refusal)} -- each
    cell on a state of its own: initial points from curves, thresholds prepared, a draw begun or not, then the call."""
    lib = _lib.require_device()
    a = _Args(lib)
    spectra = {s: _spectra(s) for s in STATES}
    seen = {}
    for kind, name, begun, f in CELLS:
        st = jointstate.CurveJointState(spectra[kind], NLIVE, None)
        assert lib.mdns_joint_init_curves(st._h, _lib.ptr(a.live_curves), 0.1, None) == 0, _lib.last_error()
        assert lib.mdns_joint_prepare(st._h, None, None, None) == 0, _lib.last_error()
        if begun:
            assert lib.mdns_backend_draw_begin(st._h, None, NDATA) == 0, _lib.last_error()
        rc, has_accepted = f(lib, a, st)
        if rc == 0:
            seen[(kind, name, begun)] = (None, None, None)
        else:
            text = _lib.last_error()
            accepted = a.accepted.value if has_accepted else None
            seen[(kind, name, begun)] = (text, accepted, bool(_curve_chunk(lib, a, st)))
        st.close()
    for s in spectra.values():
        s.close()
    a.close()
    return seen


@pytest.fixture(scope="module")
def seen():
    return observe()


def test_the_table_covers_every_cell():
    assert set(EXPECTED) == {c[:3] for c in CELLS} and len(CELLS) == len(STATES) * (len(PARAMETER_ENTRIES) + len(BACKEND_ENTRIES))
    # every statistic is refused something, and nothing is served without a draw
    for s in STATES:
        assert any(t is not None for (k, _, b), t in EXPECTED.items() if k == s and b)
        assert all(t is not None for (k, _, b), t in EXPECTED.items() if k == s and not b)


@pytest.mark.parametrize("kind,name,begun", [c[:3] for c in CELLS], ids=lambda v: str(v))
def test_refusal(kind, name, begun, seen):
    text, accepted, usable = seen[(kind, name, begun)]
    assert text == EXPECTED[(kind, name, begun)]
    if text is not None:
        assert accepted in (None, -1), "a refused call must leave *accepted == -1"
        assert usable, "a curve chunk behind the refused call failed: " + _lib.last_error()
