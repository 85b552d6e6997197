"""The score regimes of tests/score_range_cases.py hold the properties their names promise (no GPU): computed
with the oracle's searches at k = n and with float64 brute force, never with the kernels. These are conditions
on the INPUTS of tests/test_gpu_score_range.py -- if a seed fails one, the seed changes, not the condition."""
import numpy as np
import pytest

import score_range_cases as S

KEY_BUFFER = 4096          # the larger key buffer of the fused top-k: more candidates than it holds ...
MIN_DISTINCT = 2048        # ... and not the bit-identical case that the duplicate-heavy tests cover


@pytest.fixture(scope='module')
def hosts(O):
    return {name: S.host_indexes(O, name) for name in S.REGIMES}


def _range_property(name, s):
    """The regime's row of the table, in absolute terms against the documented bucket range [-0.25, 1)."""
    lo, hi = float(s.min()), float(s.max())
    if name in ('unit', 'wide_lists'):
        return S.HIST_LO < 0.0 < lo and hi < S.HIST_HI and hi - lo > 20 * S.BUCKET_WIDTH
    if name == 'across_one':     # (most queries reach 1 as well: test_regime_properties counts them)
        return 0.5 < lo < 1.0 and hi < 1.5
    if name == 'above_one':
        return lo >= 1.0
    if name == 'negated':
        return hi < -0.24
    if name == 'far_below':
        return hi < -0.25
    if name == 'tiny':
        return 2.0 ** -100 < lo and hi < 2.0 ** -30 and hi - lo < S.BUCKET_WIDTH      # normal numbers, one bucket
    if name == 'signed':
        return hi > 0.0 and lo < -0.25 and (s < 0.0).any() and (s > -0.25).any()
    if name == 'one_bucket':
        return S.HIST_LO < lo and hi < S.HIST_HI and hi - lo < S.BUCKET_WIDTH
    raise KeyError(name)


def report(h, kind):
    """Per query of one regime: (scores [nq, n] sorted by the oracle, candidates, distinct scores, the tested
    k at which the k-th and (k+1)-th score differ, those at which they are equal)."""
    n = len(h['xb'])
    Dd, I = h[kind].search(h['xq'], n, h['nlist'])
    out = []
    for q in range(len(Dd)):
        m = int((I[q] >= 0).sum())
        sc = Dd[q, :m]
        differ = [k for k in S.KS if k < m and sc[k - 1] != sc[k]]
        equal = [k for k in S.KS if k < m and sc[k - 1] == sc[k]]
        out.append((sc, m, len(np.unique(sc.view(np.uint32))), differ, equal))
    return out


def test_the_world_is_what_the_sparse_forms_need():
    xb, xq = S.world()
    assert xb.shape == (S.N, S.D) and xq.shape == (S.NQ, S.D) and xb.dtype == np.float32
    for x in (xb, xq):
        assert (np.count_nonzero(x, axis=1) == S.NNZ + S.HOT).all() and S.NNZ + S.HOT <= 64
        assert (x >= 0).all() and np.allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
    hot = np.nonzero((xb != 0).all(0))[0]
    assert len(hot) == S.HOT and (xq[:, hot] != 0).all()
    names = [r[0] for r in S.build_regimes()]
    assert tuple(names) == S.REGIMES


@pytest.mark.parametrize('name', S.REGIMES)
def test_regimes_are_scalings_and_sign_changes_of_one_world(O, hosts, name):
    """Every regime but `one_bucket` holds the control's rows times +-2^e, so the oracle's scores are the
    control's times a power of two, bit for bit: only the histogram sees a difference."""
    h = hosts[name]
    xb, xq = S.world()
    assert np.isfinite(h['xb']).all() and np.isfinite(h['xq']).all() and np.isfinite(h['cb']).all()
    assert (np.count_nonzero(h['xb'], axis=1) <= 64).all()
    in_unit = bool(((h['xb'] >= 0) & (h['xb'] < 1)).all())
    assert in_unit == (name in S.FX22_REGIMES + ('wide_lists',))
    if name == 'one_bucket':
        rel = np.abs(h['xb'].astype(np.float64) / np.where(xb[:1] != 0, xb[:1], 1.0).astype(np.float64) - 1.0)
        assert rel[:, xb[0] != 0].max() < 2e-3 and (h['xb'][:, xb[0] == 0] == 0).all()
        assert len(np.unique(h['xb'], axis=0)) == S.N
        return
    ratio_b = h['xb'][xb != 0].astype(np.float64) / xb[xb != 0].astype(np.float64)
    ratio_q = h['xq'][xq != 0].astype(np.float64) / xq[xq != 0].astype(np.float64)
    for r in (ratio_b, ratio_q):
        mant, _ = np.frexp(np.abs(r))
        assert (mant == 0.5).all()                       # exact powers of two
    assert len(np.unique(np.abs(ratio_b))) == 1 and len(np.unique(ratio_q)) == 1
    assert (len(np.unique(ratio_b)) == 2) == (name == 'signed')
    if name == 'signed':
        assert abs(int((ratio_b < 0).sum()) // (S.NNZ + S.HOT) - S.N // 2) <= 1
    if name not in ('signed', 'wide_lists'):             # same lists, same codes, scores scaled exactly
        u = hosts['unit']
        f = float(np.abs(ratio_b[0])) * float(ratio_q[0])
        for kind in ('flat', 'pq'):
            assert np.array_equal(h[kind].ids, u[kind].ids)
            if kind == 'pq':
                assert np.array_equal(h[kind].payload, u[kind].payload)
            Du, _ = u[kind].search(u['xq'], S.N, S.NLIST)
            Dh, _ = h[kind].search(h['xq'], S.N, S.NLIST)
            assert np.array_equal(np.sort(Dh, axis=1).view(np.uint32),
                                  np.sort(Du * np.float32(f), axis=1).view(np.uint32))


@pytest.mark.parametrize('kind', ['flat', 'pq'])
@pytest.mark.parametrize('name', S.REGIMES)
def test_regime_properties(O, hosts, name, kind, capsys):
    h = hosts[name]
    rows = report(h, kind)
    if kind == 'flat':       # the oracle's fp32 chain against float64 brute force: same scores, same ranges
        exact = h['xq'].astype(np.float64) @ h['xb'].astype(np.float64).T
        for q, (sc, m, *_) in enumerate(rows):
            assert m == S.N
            want = np.sort(exact[q])[::-1]
            assert np.allclose(sc.astype(np.float64), want, rtol=2e-6, atol=0.0)
            assert _range_property(name, exact[q]), (name, q, exact[q].min(), exact[q].max())
    crowd = []
    for q, (sc, m, distinct, differ, equal) in enumerate(rows):
        assert _range_property(name, sc), (name, kind, q, float(sc.min()), float(sc.max()))
        assert m > KEY_BUFFER, (name, kind, q, m)
        assert distinct > MIN_DISTINCT, (name, kind, q, distinct)
        assert differ, (name, kind, q)
        if name == 'one_bucket':
            assert equal, (name, kind, q)                # a tie at the k-th place: the id order must decide it
        crowd.append(distinct)
    if name == 'across_one':     # scores on both sides of 1 -- clamped and unclamped in one row -- for most queries
        assert sum(1 for r in rows if r[0].max() >= 1.0 and r[0].min() < 1.0) >= 12
    with capsys.disabled():
        sc_all = np.concatenate([r[0] for r in rows])
        print('\n  %-10s %-4s scores %.6g .. %.6g, %d candidates, %d .. %d distinct per query, ties at a tested k in '
              '%d of %d queries' % (name, kind, sc_all.min(), sc_all.max(), rows[0][1], min(crowd), max(crowd),
                                    sum(1 for r in rows if r[4]), len(rows)), end='')
