"""The chunk in two halves (``score_backend`` -> ``votes`` / ``set_votes`` -> ``commit_backend``) on the device states
against the same halves on ``jointstate.HostJointState``, exactly.

The host twin is fed likelihoods from the kernels the device state decides with -- the Gaussian line through the lane
kernel (chain_support.LaneScorer, as tests/test_joint.py builds its twin), the MUSE-style lines through the spectra's
own ``loglike_batch_lines``, called with the chunk's B and rows -- so votes, accepted index, fill bits, thresholds and
shelf sizes have to be equal, not close.  Both twins speak the halves only: a chunk is scored once, whole, on either
side.
"""
import numpy as np
import pytest

from massivedatans_amd import gen, jointstate, musefuse, sample
from chain_support import LaneScorer

pytestmark = pytest.mark.gpu

NLIVE, B = 8, 5


def _gauss():
    from massivedatans_amd.like import GaussLineSpectra
    data = gen.horns(130)                                   # two full tiles of 64 spectra and a tail of 2
    spectra = GaussLineSpectra(data["x"], data["y"], noise_level=0.01)
    dev = jointstate.GaussJointState(spectra, NLIVE, sample.kernel_params, fetch_rows=False, via_backend=True)
    host = jointstate.HostJointState(LaneScorer(spectra), NLIVE, 130, sample.kernel_params)
    return spectra, dev, host, sample.priortransform_batch, sample.kernel_params, 3


def _muse():
    from massivedatans_amd.like import MuseSpectra
    # 300 channels: the shortest grid of gen.muse_like on which its lines do not fall between channels
    # (tests/k2_rows_support.py), so that the candidates' likelihoods differ by more than their continuum
    data = gen.muse_like(70, 300)
    spectra = MuseSpectra(data["x"], data["y"], data["v"])
    dev = jointstate.MuseJointState(spectra, NLIVE)
    host = jointstate.HostJointState(musefuse._LinesScorer(spectra), NLIVE, 70, musefuse.kernel_params, nparams=5)
    return spectra, dev, host, musefuse.priortransform_batch, musefuse.kernel_params, 5


def _ragged(ndata, n, seed):
    return np.sort(np.random.RandomState(seed).choice(ndata, size=n, replace=False)).astype(np.int32)


def _same_state(dev, host):
    (ha, na), (hb, nb) = dev.thresholds(), host.thresholds()
    assert np.array_equal(na, nb) and np.array_equal(ha, hb)
    return ha, na


def _score(dev, host, params, rows):
    host.score_backend(params, rows)
    dev.score_backend(params, rows)
    votes = host.votes().copy()
    got = dev.votes()
    assert got.dtype == np.int32 and np.array_equal(got, votes), (got, votes)
    return votes


def _commit(dev, host):
    idx, Lrow, beats = dev.commit_backend()
    jdx, _, want = host.commit_backend()
    assert Lrow is None                                     # (no likelihood row leaves the device)
    assert idx == jdx and np.array_equal(beats, want), (idx, jdx)
    return idx, beats


CASES = [("gauss", _gauss, None), ("gauss", _gauss, _ragged(130, 70, 1)), ("muse", _muse, None), ("muse", _muse, _ragged(70, 40, 2))]


@pytest.mark.parametrize("kind,make,rows", CASES, ids=["%s-%s" % (c[0], "all" if c[2] is None else len(c[2])) for c in CASES])
def test_halves_on_the_device_equal_the_host_statement(kind, make, rows):
    spectra, dev, host, prior, kernel_params, nparams = make()
    ndata = dev.ndata
    if kind == "gauss" and rows is not None:
        assert rows[0] < 64 <= rows[-1] and (np.diff(rows) > 1).any()          # ragged, across the first tile edge
    every = np.arange(ndata) if rows is None else rows
    rng = np.random.RandomState(4)
    xs0 = prior(rng.uniform(size=(NLIVE, nparams)))
    dev.init(xs0)
    host.init(xs0)
    assert np.array_equal(dev.live_matrix(), host.live_matrix())
    a, b = dev.prepare(), host.prepare()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a few honest chunks over all data sets first: points on the shelves, thresholds that a draw from the prior can miss
    taken = 0
    for _ in range(10):
        params = kernel_params(prior(rng.uniform(size=(B, nparams))))
        _score(dev, host, params, None)
        taken += _commit(dev, host)[0] >= 0                 # (-1 where nobody voted, as a sharded draw commits)
        _same_state(dev, host)
    assert taken >= 3
    # the chunk of the test: on the host twin, some selected data set accepts a candidate and none accepts another
    for _ in range(50):
        params = kernel_params(prior(rng.uniform(size=(B, nparams))))
        host.score_backend(params, rows)
        votes = host.votes().copy()
        if votes.any() and not votes.all():
            break
    assert votes.any() and not votes.all(), "no chunk with an accepted and a refused candidate"
    before = _same_state(dev, host)
    assert np.array_equal(_score(dev, host, params, rows), votes)
    # a foreign vote: only another rank's data sets accepted a candidate that none of these accepts
    foreign = np.zeros(B, dtype=np.int32)
    foreign[np.flatnonzero(votes == 0)[0]] = 1
    dev.set_votes(foreign)
    host.set_votes(foreign)
    idx, beats = _commit(dev, host)
    assert idx == int(np.argmax(foreign)) and beats.shape == (len(every),) and not beats.any()
    after = _same_state(dev, host)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the honest commit of the same chunk
    assert np.array_equal(_score(dev, host, params, rows), votes)
    idx, beats = _commit(dev, host)
    assert idx == int(np.argmax(votes)) and beats.any()
    after = _same_state(dev, host)
    grown = np.zeros(ndata, dtype=int)
    grown[every[beats]] = 1
    assert np.array_equal(after[1], before[1] + grown)
    assert np.array_equal(dev.shelf_n, after[1])
    dev.close()
    spectra.close()
