"""The device mass-difference groups without a GPU: the numpy restatement tests/groups_ref.py -- written from the
C ABI's comment, and the source of the profile columns tests/test_gpu_groups.py compares -- equals the host code
``fdr.ssm_groups`` byte for byte on every case of tests/groups_cases.py; its profile columns are what the labels
say; the export, the switch and its errors, the parser, ``make_scorer``, and ASL_ERR_NO_DEVICE."""
import argparse
import os
import re

import numpy as np
import pytest

import groups_cases as GC
import groups_ref as R
from ann_solo_amd import fdr
from ann_solo_amd.config import Config, add_arguments

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_cases_cover_what_they_name():
    sizes = {len(md) for md, _ in GC.CASES.values()}
    assert sizes >= {0, 1, 2, 63, 64, 65, 257, 300001}
    n_mix = len(GC.CASES['realistic-min0'][0])
    assert {m for _, m in GC.CASES.values()} >= {0, 1, 2, 100, n_mix + 1}
    labels = np.unique(GC.host('realistic-min2'))
    assert labels[0] == -1 and len(labels) > 20                 # planted masses and background peaks
    assert len(np.unique(GC.host('realistic-min100'))) == 7     # -1 and the six planted masses of >= 100 SSMs
    assert (GC.host(f'realistic-min{n_mix + 1}') == -1).all()
    # a single SSM is never assigned; of two in different intervals the last in mass order is skipped
    assert GC.host('n1').tolist() == [-1] and GC.host('n2-same').tolist() == [0, 0]
    assert GC.host('n2-apart').tolist() == [-1, 0] and GC.CASES['n2-apart'][0].tolist() == [5.2, 0.3]
    assert (GC.host('only-bin0') == -1).sum() == 4 and (GC.host('only-bin99') == -1).sum() == 4
    nominal = np.rint(GC.OVER_SPAN)
    assert nominal.max() - nominal.min() + 1 == R.MAX_SPAN + 1
    with pytest.raises(OverflowError):
        R.ssm_groups(GC.OVER_SPAN, 1)


@pytest.mark.parametrize('name', GC.NAMES)
def test_restatement_equals_the_host_code(name):
    md, min_size = GC.CASES[name]
    want = GC.host(name)
    group, n_peaks, n_labels, mass, size = GC.ref(name)
    assert group.dtype == np.int32 and group.tobytes() == want.tobytes()
    assert n_labels == len(np.unique(want))
    # the profile: sizes are the counts of the UNFOLDED labels, masses the left edges of the peaks' bins
    unfolded = fdr.ssm_groups(md, 0)
    assert n_peaks == len(mass) == len(size) and size.dtype == np.int64 and mass.dtype == np.float64
    assert n_peaks >= (unfolded.max() + 1 if len(md) else 0)
    assert size.tobytes() == np.bincount(unfolded[unfolded >= 0], minlength=n_peaks).astype(np.int64).tobytes()
    assert mass.tobytes() == _bins_of_peaks(md).tobytes()


def _bins_of_peaks(md) -> np.ndarray:
    """``bins[peaks]`` of every interval the host code closes, in its order, from scipy as the host code calls it."""
    import scipy.signal
    out = []
    nominal = np.rint(md)
    for g in np.unique(nominal):
        x = md[nominal == g]
        if len(md) == 1 or (g == nominal.max() and len(x) == 1):
            continue
        bins = np.linspace(g - 0.5, g + 0.5, 101)
        peaks, _ = scipy.signal.find_peaks(np.histogram(x, bins=bins)[0], prominence=(None, None))
        out.append(bins[peaks])
    return np.concatenate(out) if out else np.zeros(0)


def test_edges_are_numpys_linspace():
    for g in GC.EDGE_NOMINALS + (2, -32768, 32767):
        assert R.edges(float(g)).tobytes() == np.linspace(g - 0.5, g + 0.5, 101).tobytes()
    for g in GC.CONTRACTION_NOMINALS:
        assert (R.edges(float(g)) != R.edges_contracted(float(g))).any()


def test_restatement_refuses_what_the_entry_point_refuses():
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='non-finite'):
            R.ssm_groups(np.array([0.1, bad, 0.2]), 1)
    with pytest.raises(ValueError, match='min_group_size'):
        R.ssm_groups(np.array([0.1, 0.2]), -1)


# ------------------------------------------------------------------ the switch
def test_the_switch_and_its_errors():
    assert Config().device_groups is False
    p = argparse.ArgumentParser()
    add_arguments(p)
    assert p.parse_args([]).device_groups is False
    ns = p.parse_args(['--device_fdr', '--device_groups'])
    cfg = Config.from_reference(ns)
    assert cfg.device_groups is True and cfg.device_fdr is True and cfg.device_qvalues is False
    with pytest.raises(ValueError, match='device_groups.*needs device_fdr'):
        Config(device_groups=True)
    with pytest.raises(ValueError, match='sharded'):
        Config(device_fdr=True, device_groups=True, num_gpus=2)
    assert Config(device_fdr=True, device_groups=True, num_gpus=1).device_groups


def test_make_scorer_hands_the_keyword_on():
    for kw, cls in ((dict(), fdr.CosineTDC), (dict(model='svm'), fdr.PercolatorTDC),
                    (dict(model='rf', device_forest=True), fdr.ForestTDC)):
        off = fdr.make_scorer(Config(device_fdr=True, **kw), device='cuda:0')
        on = fdr.make_scorer(Config(device_fdr=True, device_groups=True, fdr=0.05, **kw), device='cuda:0')
        both = fdr.make_scorer(Config(device_fdr=True, device_groups=True, device_qvalues=True, **kw), device='cuda:0')
        assert isinstance(off, cls) and isinstance(on, cls)
        assert off.groups is None and on.groups == 'device' and on.qvalues is None and on.device == 'cuda:0'
        assert both.groups == 'device' and both.qvalues == 'device' and on.fdr == 0.05
        assert off.group_profile is None and on.group_profile is None
    with pytest.raises(ValueError, match='groups'):
        fdr.PercolatorTDC(groups='host')
    with pytest.raises(ValueError, match='groups'):
        fdr.CosineTDC(groups='gpu')


def test_no_hash_knows_the_switch():
    from ann_solo_amd.spectral_library import SpectralLibrary
    out = []
    for kw in (dict(device_fdr=True), dict(device_fdr=True, device_groups=True)):
        sl = SpectralLibrary.__new__(SpectralLibrary)
        sl.config = Config.open_search(**kw)
        out.append((sl._get_hyperparameter_hash(), sl._get_index_hash()))
    assert out[0] == out[1]


def test_entry_point_is_exported_and_declared():
    from ann_solo_amd import _lib
    assert 'asl_ssm_groups' in _lib.EXPORTS and hasattr(_lib.lib(), 'asl_ssm_groups')
    with open(os.path.join(HERE, '..', 'include', 'annsolo_mi.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+asl_ssm_groups\s*\(', header)
    assert int(re.search(r'#define\s+ASL_GROUPS_MAX_SPAN\s+(\d+)', header).group(1)) == _lib.GROUPS_MAX_SPAN == R.MAX_SPAN


def test_what_is_checked_before_the_device_is_touched():
    from ann_solo_amd import _lib
    md, group = np.array([0.1, 0.2]), np.full(2, 77, np.int32)
    L = _lib.lib()
    assert L.asl_ssm_groups(_lib.ptr(md), -1, 1, _lib.ptr(group), None, None, None, None) == -1      # ASL_ERR_INVALID
    assert L.asl_ssm_groups(_lib.ptr(md), 2, -1, _lib.ptr(group), None, None, None, None) == -1
    assert L.asl_ssm_groups(_lib.ptr(md), 1 << 31, 1, _lib.ptr(group), None, None, None, None) == -4  # .._CAPACITY
    assert (group == 77).all()
    g, n_labels, mass, size = _lib.ssm_groups(np.zeros(0), 5, profile=True)       # n == 0 launches nothing
    assert g.shape == (0,) and g.dtype == np.int32 and n_labels == 0 and len(mass) == len(size) == 0


def _has_device() -> bool:
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_device(), reason='checks the behaviour without a HIP device')
def test_groups_need_a_device():
    from ann_solo_amd import _lib
    md, group = np.array([0.1, 0.2]), np.full(2, 77, np.int32)
    L = _lib.lib()
    assert L.asl_ssm_groups(_lib.ptr(md), 2, 1, _lib.ptr(group), None, None, None, None) == -2       # ASL_ERR_NO_DEVICE
    with pytest.raises(_lib.AnnSoloMiError) as err:
        _lib.ssm_groups(md, 1)
    assert err.value.code == -2 and (group == 77).all()
