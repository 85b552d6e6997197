"""``asl_tdc_qvalues`` (csrc/tdc.hip) against the host code of ann_solo_amd/fdr.py, byte for byte, on every case
of tests/tdc_cases.py; its errors; the three scorers with ``qvalues='device'`` against themselves without; and
``Config.device_qvalues`` end to end on the small library of test_gpu_device_fdr.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decoy_cases as DC     # noqa: E402
import decoy_ref            # noqa: E402
import fdr_cases as FC       # noqa: E402
import tdc_cases as TC       # noqa: E402
from fake_reader import FakeReader, FakeSpectrum   # noqa: E402

DEV = 'cuda:0'
NAMES = [name for name, _ in TC.CASE_IDS]


def _on_device(a):
    return None if a is None else torch.as_tensor(np.array(a)).to(DEV)      # (a copy: the cases are read-only)


@pytest.mark.parametrize('name', NAMES)
def test_q_and_labels_equal_the_host_code(name):
    from ann_solo_amd import _lib
    score, target, group, use, desc = TC.get(name)
    want = TC.host_q(name)
    q = _lib.tdc_qvalues(score, target, group, use, desc)
    assert isinstance(q, np.ndarray) and q.dtype == np.float64 and q.tobytes() == want.tobytes()
    dev = [_on_device(a) for a in (score, target, group, use)]
    qd = _lib.tdc_qvalues(*dev, desc)
    assert qd.is_cuda and qd.dtype == torch.float64 and qd.cpu().numpy().tobytes() == want.tobytes()
    for level in (0.01, 0.5):
        labels = TC.host_labels(name, level)
        q, lab = _lib.tdc_qvalues(score, target, group, use, desc, fdr=level)
        assert q.tobytes() == want.tobytes() and lab.dtype == np.int8 and lab.tobytes() == labels.tobytes()
        qd, labd = _lib.tdc_qvalues(*dev, desc, fdr=level)
        assert labd.is_cuda and labd.dtype == torch.int8
        assert qd.cpu().numpy().tobytes() == want.tobytes() and labd.cpu().numpy().tobytes() == labels.tobytes()
    # a second call: the same bytes
    assert _lib.tdc_qvalues(*dev, desc).cpu().numpy().tobytes() == want.tobytes()


def _raw(score, target, use, n, desc, fdr, q, label):
    from ann_solo_amd import _lib
    return _lib.lib().asl_tdc_qvalues(_lib.ptr(score), _lib.ptr(target), None, _lib.ptr(use), n, desc, fdr,
                                      _lib.ptr(q), _lib.ptr(label))


@pytest.mark.parametrize('device', [False, True])
def test_errors_leave_the_outputs_untouched(device):
    from ann_solo_amd import _lib
    rng = np.random.default_rng(3)
    n = 1500
    score, target = rng.random(n), (rng.random(n) < 0.5).astype(np.uint8)
    use = np.ones(n, np.uint8)
    bad = score.copy()
    bad[1234] = np.nan
    move = _on_device if device else (lambda a: a)
    q0, l0 = np.full(n, -7.0), np.full(n, 99, np.int8)
    for what, (s, u, n_, desc, level, with_label) in dict(
            negative_n=(score, use, -1, 1, 0.01, True), desc_2=(score, use, n, 2, 0.01, True),
            nan_fdr=(score, use, n, 1, np.nan, True), negative_fdr=(score, use, n, 1, -0.25, True),
            nan_score=(bad, use, n, 1, 0.01, True), nan_score_no_label=(bad, None, n, 0, 0.01, False)).items():
        q, lab = move(q0.copy()), move(l0.copy())
        rc = _raw(move(s), move(target), None if u is None else move(u), n_, desc, level, q, lab if with_label else None)
        assert rc == -1, what                               # ASL_ERR_INVALID
        assert _lib.lib().asl_last_error()
        back = (lambda a: a.cpu().numpy()) if device else (lambda a: a)
        assert back(q).tobytes() == q0.tobytes() and back(lab).tobytes() == l0.tobytes(), what
    with pytest.raises(_lib.AnnSoloMiError):
        _lib.tdc_qvalues(move(bad), move(target))
    # a NaN fdr without label is not read; a NaN in an UNUSED row is legal
    q = move(q0.copy())
    assert _raw(move(score), move(target), None, n, 1, np.nan, q, None) == 0
    skip = use.copy()
    skip[1234] = 0
    q, lab = _lib.tdc_qvalues(move(bad), move(target), use=move(skip), fdr=0.5)
    q, lab = (q.cpu().numpy(), lab.cpu().numpy()) if device else (q, lab)
    keep = np.arange(n) != 1234
    from ann_solo_amd import fdr
    assert np.isnan(q[1234]) and lab[1234] == 0
    assert q[keep].tobytes() == fdr.tdc_qvalues(score[keep], target[keep].astype(bool)).tobytes()
    # n == 0: legal, nothing is written
    assert _lib.tdc_qvalues(np.zeros(0), np.zeros(0, bool)).shape == (0,)


# ------------------------------------------------------------------------------------------ the scorers
def _same_trace(dev, ref, rounds=10):
    assert not dev.fallback and not ref.fallback and len(dev.trace) == len(ref.trace) == 3
    for x, y in zip(dev.trace, ref.trace):
        assert x['grid'] == y['grid'] and len(x['labels']) == len(y['labels']) == rounds
        for la, lb in zip(x['labels'], y['labels']):
            assert isinstance(la, np.ndarray) and la.dtype == lb.dtype and la.tobytes() == lb.tobytes()


def test_percolator_with_device_qvalues_is_percolator():
    from ann_solo_amd import fdr
    a, b = FC.robust_table(), FC.robust_table()
    dev, ref = fdr.PercolatorTDC(device=DEV, qvalues='device'), fdr.PercolatorTDC(device=DEV)
    dev(a, 'std')
    ref(b, 'std')
    _same_trace(dev, ref)
    assert a.score.tobytes() == b.score.tobytes() and a.q.tobytes() == b.q.tobytes()
    assert (a.q <= 0.01).sum() > 1500


def test_forest_with_device_qvalues_is_forest():
    from ann_solo_amd import fdr
    a, b = FC.robust_table(), FC.robust_table()
    dev, ref = fdr.ForestTDC(device=DEV, trees=16, qvalues='device'), fdr.ForestTDC(device=DEV, trees=16)
    dev(a, 'std')
    ref(b, 'std')
    _same_trace(dev, ref)
    assert a.score.tobytes() == b.score.tobytes() and a.q.tobytes() == b.q.tobytes()


def _grouped_table(seed=8):
    """A table whose mass differences fall into four narrow clusters -- three of them above ``min_group_size``
    = 40, one of 12 rows below it -- and a scattered residue: ``ssm_groups`` gives three groups and -1."""
    from ann_solo_amd.spectral_library import SSMTable
    rng = np.random.default_rng(seed)
    sizes = {0.0: 300, 15.9949: 180, 79.9663: 90, 42.0106: 12}
    delta = np.concatenate([np.full(k, d) + rng.normal(0, 0.0015, k) for d, k in sizes.items()]
                           + [rng.uniform(-30, 120, 60)])
    n = len(delta)
    delta = delta[rng.permutation(n)]
    lib_pmz = rng.uniform(400, 900, 50)
    lib_decoy = rng.random(50) < 0.4
    lib_row = rng.integers(0, 50, n).astype(np.int32)
    lmeta = {2: [dict(identifier=i, peptide='P', precursor_mz=float(lib_pmz[i]),
                      **({'is_decoy': True} if lib_decoy[i] else {})) for i in range(50)]}
    qmeta = {2: [dict(identifier=i, index=i, precursor_mz=float(lib_pmz[lib_row[i]] + delta[i] / 2),
                      precursor_charge=2) for i in range(n)]}
    t = SSMTable(qmeta, lmeta)
    t.charge = np.full(n, 2, np.int32)
    t.qrow = np.arange(n, dtype=np.int64)
    t.lib_row = lib_row
    t.score = np.round(rng.random(n), 2)          # runs of equal cosines inside the groups
    t.q = np.full(n, np.nan)
    t.batch = np.zeros(n, np.int32)
    t.pos = np.arange(n, dtype=np.int32)
    return t


def test_cosine_tdc_open_with_device_qvalues_is_cosine_tdc():
    from ann_solo_amd import fdr
    a, b = _grouped_table(), _grouped_table()
    ids, counts = np.unique(fdr.ssm_groups(a.mass_diffs(), 40), return_counts=True)
    assert ids[0] == -1 and len(ids) >= 4 and (counts[1:] >= 40).all()      # a residue and three groups
    dev, ref = fdr.CosineTDC(40, qvalues='device', device=DEV), fdr.CosineTDC(40)
    for mode in ('open', 'std'):
        cos = a.score.copy()
        assert dev(a, mode) is None and ref(b, mode) is None
        assert a.q.tobytes() == b.q.tobytes() and a.score.tobytes() == b.score.tobytes()
        assert np.isfinite(a.q).sum() == (~a.is_decoy()).sum() > 200
        a.score, b.score = cos.copy(), cos.copy()
    assert dev.n_groups == ref.n_groups == len(ids)


# ------------------------------------------------------------------------------------------ end to end
def _library(n=400, seed=33):
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        c = DC.make_case(rng, int(rng.integers(9, 22)), 2, int(rng.integers(60, 140)), 0.02, 'Da', frac=0.8)
        mass = float(c['masses'].sum()) + decoy_ref.H2O
        specs.append(FakeSpectrum(f'lib{i:04d}', (mass + 2 * decoy_ref.PROTON) / 2, 2, c['mz'], c['intensity'], None,
                                  c['peptide'], retention_time=float(i)))
    return specs


def _queries(specs, seed=34):
    """Noisy copies of the first 300 library spectra (every third with its precursor moved by a modification
    mass, for the open level) and 300 spectra of peptides the library does not hold, at precursor masses it
    does: those match targets and decoys alike."""
    rng = np.random.default_rng(seed)
    out = []
    for j, s in enumerate(specs[:300]):
        keep = rng.random(len(s.mz)) < 0.9
        mz = np.sort((s.mz[keep] + rng.normal(0, 0.003, int(keep.sum()))).astype(np.float32))
        shift = (15.9949 if j % 3 == 0 else 0.0) / 2
        out.append(FakeSpectrum(f'scan={j}', s.precursor_mz + shift, 2, mz,
                                s.intensity[keep] * rng.uniform(0.8, 1.25, int(keep.sum())), index=j))
    for j, s in enumerate(_library(300, seed + 1)):
        host = specs[int(rng.integers(len(specs)))]
        out.append(FakeSpectrum(f'scan={300 + j}', host.precursor_mz * (1 + 2e-6 * rng.normal()), 2, s.mz, s.intensity,
                                index=300 + j))
    return out


def test_the_switch_end_to_end(tmp_path):
    from ann_solo_amd import fdr
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    from ann_solo_amd.spectral_library import SpectralLibrary
    specs = _library()
    base = dict(num_list=8, num_probe=8, num_candidates=64, kmeans_niter=4, fragment_mz_tolerance=0.02,
                decoy_tolerance_unit='Da', seed=5, min_mz_range=100.0, device_decoys=True, fdr=0.05,
                fdr_min_group_size=20, precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm',
                device_fdr=True, model='svm')
    tables = []
    for k, extra in enumerate((dict(), dict(device_qvalues=True))):
        d = tmp_path / f'lib{k}'
        d.mkdir()
        eng = SpectralLibrary(FakeReader(specs, str(d / 'lib.splib')), config=Config.open_search(**base, **extra),
                              device=DEV)
        try:
            assert isinstance(eng._score_ssms, fdr.PercolatorTDC)
            assert eng._score_ssms.qvalues == ('device' if extra else None)
            qs, qmeta = pack_queries(iter(_queries(specs)), eng.config, eng.device)
            t = eng.search_packed(qs, qmeta, eng.library_meta)
            tables.append(eng.search_packed(qs, qmeta, eng.library_meta))
        finally:
            eng.shutdown()
    a, b = tables
    assert len(a) == len(b) > 100
    for name in ('charge', 'qrow', 'lib_row', 'open_level'):        # the accepted identifications
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    assert a.score.tobytes() == b.score.tobytes() and a.q.tobytes() == b.q.tobytes()
