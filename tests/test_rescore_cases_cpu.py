"""The rescoring case generator (tests/rescore_cases.py) really plants what the GPU tests of
test_gpu_rescore_numeric.py rely on: counted from the oracle's matched pairs, every regime holds
thousands of matched peaks and at least a thousand of them on the edge of their window. Without
this the GPU tests could pass by planting nothing."""
import numpy as np
import pytest

import rescore_cases as RC


@pytest.mark.parametrize('number', RC.REGIMES)
def test_regime_plants_matches_on_the_window_edge(O, number):
    n_match = n_edge = n_pairs = 0
    for block in RC.regime_blocks(number):
        m, e = RC.boundary_stats(O, block)
        print(f'{block.name}: {block.nlib} pairs, {m} matched peaks, {e} within 4 ulp of the edge')
        assert m > 0 and e > 0, block.name          # no block of a regime is empty
        n_match, n_edge, n_pairs = n_match + m, n_edge + e, n_pairs + block.nlib
    print(f'regime {number}: {n_pairs} pairs, {n_match} matched, {n_edge} on the edge')
    assert n_match >= 5000
    assert n_edge >= 1000


@pytest.mark.parametrize('number', RC.REGIMES)
def test_regime_spectra_are_well_formed(number):
    for block in RC.regime_blocks(number):
        qo, qmz, qit, _, qpmz, _ = block.queries
        lo, lmz, lit, lch, lpmz, lz = block.library
        assert set(np.diff(qo).tolist()) <= set(RC.QN)
        assert np.diff(lo).max() <= RC.CN_MAX and np.diff(lo).min() >= 1
        for o, mz in ((qo, qmz), (lo, lmz)):
            assert np.all(np.isfinite(mz)) and np.all(mz > 0)
            inner = np.ones(len(mz), bool)
            inner[o[1:-1]] = False                   # first peak of a spectrum: no predecessor
            assert np.all(np.diff(mz)[inner[1:]] >= 0), 'peaks ascend'
        for q in range(block.nq):                    # query peaks at least 8 tol apart
            d = np.diff(qmz[qo[q]:qo[q + 1]].astype(np.float64))
            assert d.size == 0 or d.min() >= 8 * block.tol
        assert np.all(qpmz > 0) and np.all(lpmz > 0)
        assert np.all(np.isfinite(qit)) and np.all(np.isfinite(lit)) and np.all(lit >= 0)
        assert np.all(lch <= lz[np.repeat(np.arange(block.nlib), np.diff(lo))])
        rows, off = RC.grouped_lists(block)
        assert np.all(np.diff(off) == min(40, block.nlib))
        for q in range(block.nq):                    # a query's own candidates are in its list
            assert set(np.nonzero(block.owner == q)[0]) <= set(rows[off[q]:off[q + 1]].tolist())


def test_regimes_reach_their_targets():
    """The precursor mass differences and m/z ranges the regimes are named for."""
    def pmd(block):
        _, _, _, _, lpmz, lz = block.library
        return (block.queries[4][block.owner] - lpmz) * lz
    r1 = np.concatenate([pmd(b) for b in RC.regime_blocks(1)])
    assert np.abs(r1).max() > RC.RS_MD_ENV and np.any((np.abs(r1) < RC.RS_MD_ENV) & (np.abs(r1) > RC.RS_MD_ENV - 1))
    assert all(np.all(pmd(b) < 0) and b.queries[1].max() <= 5.0 for b in RC.regime_blocks(2))
    t = RC.threshold_tol(2600.0)
    tols = sorted(b.tol for b in RC.regime_blocks(3))
    assert tols[0] == 0.00076 and tols[1] == 0.00077 and tols[2] < t < tols[3]
    assert RC.margin(tols[3], 2600.0) <= RC.RS_MARGIN_MAX < RC.margin(tols[2], 2600.0)
    assert max(b.queries[1].max() for b in RC.regime_blocks(4)) > 90000
    r5 = np.concatenate([pmd(b) for b in RC.regime_blocks(5)])
    for a in (2e4, 1e5):
        for sg in (-1, 1):
            assert np.any(np.abs(r5 - sg * a) < 1e-6 * a)
    assert set(np.concatenate([b.library[5] for b in RC.regime_blocks(5)]).tolist()) == {4, 30}


def test_generator_envelope_is_the_kernels():
    """The envelope the regimes are placed around is the one csrc/rescore.hip compiles."""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           'ann_solo_amd', 'csrc', 'rescore.hip')) as f:
        src = f.read()
    assert float(re.search(r'constexpr double RS_MD_ENV = ([0-9.e+-]+);', src).group(1)) == RC.RS_MD_ENV
    assert float(re.search(r'constexpr double RS_MARGIN_MAX = ([0-9.e+-]+);', src).group(1)) == RC.RS_MARGIN_MAX
    # (a tripwire on the expression, whatever its layout)
    assert 'return1e-3+(0.5/tol)*6.0e-8*(RS_MD_ENV+3.0*(q_abs+tol));' in re.sub(r'\s+', '', src)
    assert RC.margin(0.02, 1900.0) == 1e-3 + (0.5 / 0.02) * 6.0e-8 * (4096.0 + 3.0 * (1900.0 + 0.02))


@pytest.mark.parametrize('shifted', [False, True])
def test_gate_cases_tell_an_off_by_one_gate(shifted):
    """The exact-sum cases of the GPU test (RC.gate_case): up to an exponent spread of 23 the fp64
    sum of the products is the same in EVERY order (24 + 23 + 6 = 53 bits) -- that is what lets
    the kernels keep an unordered sum -- and from 24 on it is not: with several small products
    there are arrival orders, for some cases the candidate's own peak order, whose sum differs from
    the sorted-order sum the reference computes. A gate one binade too wide would let those
    through, and the GPU test would see the last bit. (ONE small product, the issue's case,
    sees a single rounding in any order and cannot tell: asserted here too, so nobody relies on it.)"""
    _, library, owner, meta = RC.gate_case(shifted)
    rng = np.random.default_rng(5)
    differ = {}
    for r, (cn, z, d, k, where) in enumerate(meta):
        p = RC.gate_products(library, r, shifted)
        e = (p.view(np.uint32) >> 23) & 0xff
        assert int(e.max()) - int(e.min()) in ((d, d + 1) if shifted else (d,))    # 2/3 may cross a binade
        want = RC.sum_in_order(np.sort(p)[::-1])
        orders = [np.arange(cn), np.arange(cn)[::-1]] + [rng.permutation(cn) for _ in range(40)]
        n = sum(RC.sum_in_order(p[o]) != want for o in orders)
        peak_order = RC.sum_in_order(p) != want
        spread = int(e.max()) - int(e.min())
        if spread <= 23:
            assert n == 0, (r, meta[r])
        differ.setdefault((spread, cn, k, where), []).append((n, peak_order))
    at24 = {key: v for key, v in differ.items() if key[0] == 24 and key[1] == 64 and key[2] >= 2}
    assert len(at24) >= 4                                   # 2 and 8 small products, first / random / last
    for key, v in at24.items():                             # every such shape: some order differs
        assert sum(n for n, _ in v) > 0, key
    assert sum(po for v in at24.values() for _, po in v) >= 4      # the candidate's own peak order too
    # one small product: the same single rounding in every order, up to spread 25
    assert all(n == 0 for (sp, cn, k, where), v in differ.items() if k == 1 and sp <= 25 for n, _ in v)
