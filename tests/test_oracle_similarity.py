"""CPU checks of the oracle's SSM similarity features (oracle/asl_oracle_sim.c; reference
spectrum_similarity.py:13-730 as called by utils.py:344-456):
  * the constants the reference's own tests hold (src/tests/spectrum_similarity_test.py,
    copied as data into tests/golden/similarity_expected.json) on the reference's fixtures,
  * tests/golden/ssm_features_golden.npz = the reference module run on seeded SSMs,
  * tests/golden/ssm_features_edges.npz = the reference module on one SSM per branch of the
    kernel (more than 64 / 128 matched peaks, Kendall's switches, ties, zeros, top = 1 / 3 / 12).
The reference sums float32 arrays (NumPy pairwise order); the restatement carries doubles,
hence 1e-5 (north star tolerance for scores)."""
import json
import math
import os

import numpy as np
import pytest

from sim_common import COLUMN, NO_MATCH, EdgeCases, check_features, check_top_features, kat_case

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_test_constants(O):
    exp = json.load(open(os.path.join(HERE, 'golden', 'similarity_expected.json')))
    kat = np.load(os.path.join(HERE, 'golden', 'similarity_kat.npz'))
    checked = 0
    cache = {}
    for e in exp:
        top = e['fixture'].endswith('_top')
        name = e['fixture'][:-4] if top else e['fixture']
        col = COLUMN.get((e['method'], e['args'].replace('"', "'") if e['method'] != 'hypergeometric_score'
                          else '', top))
        if col is None:
            continue                      # variant that utils._compute_ssm_features never requests
        hg = e['method'] == 'hypergeometric_score'
        key = (name, hg)
        if key not in cache:
            q_mz, q_int, l_mz, l_int, pm = kat_case(kat, name)
            args = (101, 1500, 0.1) if hg else (11, 2010, 0.04)   # params of test_hypergeometric_score
            cache[key] = O.ssm_features(q_mz, q_int, l_mz, l_int, pm, *args)
        got = cache[key][col]
        if np.isinf(e['value']):
            assert got == e['value'], e
        else:
            assert got == pytest.approx(e['value'], rel=1e-5, abs=2e-6), e
        checked += 1
    assert checked >= 60


def test_golden_features(O):
    g = np.load(os.path.join(HERE, 'golden', 'ssm_features_golden.npz'))
    qo, lo, po = g['q_offsets'], g['l_offsets'], g['pm_offsets']
    for c in range(len(g['features'])):
        got = O.ssm_features(g['q_mz'][qo[c]:qo[c + 1]], g['q_intensity'][qo[c]:qo[c + 1]],
                             g['l_mz'][lo[c]:lo[c + 1]], g['l_intensity'][lo[c]:lo[c + 1]],
                             g['pm_pairs'][po[c]:po[c + 1]])
        check_features(got, g['features'][c], f'case {c}')


def test_degenerate_inputs(O):
    """No matches (the reference skips such SSMs, the calculator still defines the values),
    a single match, fewer library peaks than `top`."""
    mz = np.linspace(100, 1000, 12).astype(np.float32)
    it = (np.arange(12) + 1).astype(np.float32)
    it /= np.linalg.norm(it)
    f = O.ssm_features(mz, it, mz, it, np.zeros((0, 2), np.uint32))
    assert f[0] == 0 and f[2] == 0 and np.isinf(f[9]) and np.isinf(f[23]) and f[30] == 1.0
    assert f[16] == 0 and f[26] == 0 and np.isinf(f[31])
    f = O.ssm_features(mz, it, mz, it, np.array([[3, 3]], np.uint32))
    assert f[2] == 1 and f[16] == 0.0 and f[0] == pytest.approx(float(it[3]) ** 2, rel=1e-6)
    f = O.ssm_features(mz[:4], it[:4], mz[:4], it[:4], np.array([[0, 0], [1, 1]], np.uint32))
    assert f[5] == pytest.approx(0.5) and f[4] == pytest.approx(0.5)     # top >= n_library: all peaks


def test_edge_fixture_features(O):
    """Every case of the edge fixture, all 33 columns, and the `*_top` columns at top = 1, 3, 12
    (where the reference defines them: its correlations raise on the single point of a matched
    top = 1 peak, the oracle gives 0 there)."""
    E = EdgeCases()
    assert E.n >= 30 and len(set(E.names)) == E.n
    n_top = 0
    for c in range(E.n):
        q_mz, q_int, l_mz, l_int, pm = E.case(c)
        check_features(O.ssm_features(q_mz, q_int, l_mz, l_int, pm), E.features[c], E.names[c])
        for ti, t in enumerate(E.tops):
            want = E.features_top[c, ti]
            if E.nl[c] < 13:
                assert np.isnan(want).all()
                continue
            assert set(E.top_columns[np.isnan(want)]) <= ({27, 29} if t == 1 else set())
            check_top_features(O.ssm_features(q_mz, q_int, l_mz, l_int, pm, top=t), want,
                               E.top_columns, f'{E.names[c]} top={t}')
            n_top += 1
    assert n_top >= 3 * 20
    # the fixture holds what its labels say
    f = E.features[E.names.index('underflow_171_monotone')]
    assert f[2] == 171 and f[16] == np.inf
    f = E.features[E.names.index('underflow_170_monotone')]
    assert f[16] == pytest.approx(705.9, abs=0.1)
    for nm in ('half_n4_dis3', 'half_n5_dis5', 'n2', 'n1', 'constant_query_n6'):
        assert E.features[E.names.index(nm)][16] == 0.0, nm
    assert max(E.cnt) == 200 and max(E.nq) == 256
    lib_order = [bool((np.diff(E.case(c)[4][:, 1].astype(np.int64)) > 0).all()) for c in range(E.n)]
    assert [E.names[c] for c in range(E.n) if not lib_order[c]] == ['permuted_pairs_n15']


def test_degenerate_inputs_empty_spectra_and_short_libraries(O):
    """Values only the restatement defines (the reference never sees an SSM without matches, and
    its argpartition raises for a library shorter than `top`): empty spectra behind a valid row
    are the no-match row; a library of 3 or 4 peaks is all `top`."""
    mz = np.linspace(100, 1000, 12).astype(np.float32)
    it = (np.arange(12) + 1).astype(np.float32)
    it /= np.linalg.norm(it)
    e = np.zeros(0, np.float32)
    none = np.zeros((0, 2), np.uint32)
    for tag, (qa, qb, la, lb) in {'no match': (mz, it, mz, it), 'empty query': (e, e, mz, it),
                                  'empty library': (mz, it, e, e), 'both empty': (e, e, e, e)}.items():
        f = O.ssm_features(qa, qb, la, lb, none)
        for col, want in NO_MATCH.items():
            assert f[col] == want, (tag, col, f[col])
        # no bin shared by chance: C(N - nl, nl) / C(N, nl); -log(1 - that), capped at 100
        nl, N = len(la), O.get_dim(11, 2010, 0.04)[0]
        lc = lambda n, k: math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)
        p_any = -math.expm1(lc(N - nl, nl) - lc(N, nl))
        assert f[15] == (100.0 if nl == 0 else pytest.approx(-math.log(p_any), rel=1e-6)), (tag, f[15])
    pm = np.array([[0, 0], [2, 1], [5, 2]], np.uint32)
    for nl in (3, 4):
        li = it[:nl] / np.linalg.norm(it[:nl])
        f = O.ssm_features(mz, it, mz[:nl], li, pm)
        assert np.isfinite(f).all(), (nl, f)
        assert f[2] == 3 and f[4] == pytest.approx(3 / nl) and f[5] == pytest.approx(3 / nl)
        # every library peak is a top peak: the top columns are the full ones (cosine renormalised)
        for top_col, col in ((8, 7), (10, 9), (12, 11), (22, 21), (27, 26), (29, 28)):
            assert f[top_col] == f[col], (nl, top_col)
        a, b = it[pm[:, 0]].astype(np.float64), li[pm[:, 1]].astype(np.float64)
        assert f[1] == pytest.approx(a @ b / np.sqrt((a @ a) * (b @ b)), rel=1e-12)
