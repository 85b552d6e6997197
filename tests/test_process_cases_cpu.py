"""CPU checks over the named edge cases of process_cases: the numpy definition
(process_ref.numpy_process) meets what every case states it was built to hit, and the oracle's
restatement (oracle/asl_oracle.c: orc_process_spectrum), which the device kernel is held to
bit for bit, equals the definition on every one of them."""
import numpy as np
import pytest

from process_cases import CASES, oracle_args
from process_ref import numpy_process

_REF = {}


def ref(c):
    """numpy_process of a case, computed once and shared."""
    if c.name not in _REF:
        _REF[c.name] = numpy_process(c.mz, c.intensity, c.precursor_mz, c.precursor_charge, **c.cfg)
    return _REF[c.name]


def test_case_list_is_complete():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names) and 80 <= len(names) <= 130
    for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096):
        for mp in (1, 50, 255, 256):
            assert f'sort_n{n}_mp{mp}' in names
    for lo, hi in ((1, 256), (257, 1024), (1025, 4096)):      # every scaling at every sort size
        got = {c.cfg['scaling'] for c in CASES if c.name.startswith('sort_') and lo <= len(c.mz) <= hi}
        assert got == {'rank', 'sqrt', None}
    assert max(len(c.mz) for c in CASES) == 4096
    assert all((np.diff(c.mz) >= 0).all() for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_numpy_definition_meets_expectation(c):
    ok, mz, it, src = ref(c)
    assert ok == c.exp['valid']
    if not ok:
        return
    assert len(mz) == len(it) == len(src) and (np.diff(src) > 0).all()
    if 'count' in c.exp:
        assert len(mz) == c.exp['count']
    if 'src' in c.exp:
        assert np.array_equal(src, c.exp['src'])
    if 'mz' in c.exp:
        assert np.array_equal(mz, c.exp['mz'])
    assert abs(float(np.linalg.norm(it.astype(np.float64))) - 1) < 1e-6


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_oracle_equals_numpy_definition(O, c):
    ok2, m2, i2, s2 = ref(c)
    ok, om, oi, src = O.process_spectrum(c.mz, c.intensity, c.precursor_mz, c.precursor_charge,
                                         **oracle_args(c.cfg))
    assert ok == ok2
    if not ok:
        assert len(om) == 0
        return
    assert np.array_equal(om, m2) and np.array_equal(src, s2)
    # the fmaf chain rounds once per step, the numpy emulation twice at most: 1 ulp
    # (test_oracle_process.py's bound)
    assert np.allclose(oi, i2, rtol=3e-7, atol=0)
