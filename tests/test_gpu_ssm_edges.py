"""The SSM feature kernel (csrc/similarity.hip) at the shapes its other tests never reach: more
than 64 and more than 128 matched peaks, each branch of Kendall's p-value, tie groups, zero
intensities, `top` other than 5, short and empty spectra, the 128 -> 256 peak re-launch, the
batch layout, and the rule for peak match counts (include/annsolo_mi.h).

References: tests/golden/ssm_features_edges.npz (the reference's calculator, rel 1e-5 / abs
5e-6, the project's tolerance for scores) and the oracle restatement in double precision at
rel 1e-9 / abs 1e-11, the bound the other GPU similarity tests hold on spectra of at most 50
peaks. Measured on an MI355X over the edge fixture (test_edge_fixture_parity prints it): the
largest deviation from the oracle, in units of that bound, is 2.1e-3 (column 15, the
hypergeometric score), 3.0e-5 for Kendall's -log p (column 16), below 1e-5 for every other
column and 0 (equal bits) for 17 of the 33; with top = 1 / 3 / 12 at most 2.7e-6 (column 27).
No column needs a bound of its own, at 200 matched peaks and on the asymptotic path either.
"""
import numpy as np
import pytest

from sim_common import NO_MATCH, EdgeCases, check_features, check_top_features

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rel=1e-9, abs_=1e-11)


def _pack(offsets, mz, inten):
    from ann_solo_amd.packed import PackedSpectra
    n = len(offsets) - 1
    return PackedSpectra.from_numpy(offsets, mz, inten, None, np.full(n, 500.0), np.full(n, 2))


def _pack_list(mzs, ints):
    off = np.concatenate([[0], np.cumsum([len(m) for m in mzs])]).astype(np.int32)
    cat = lambda xs: np.concatenate([np.asarray(x, np.float32) for x in xs]) if len(xs) else np.zeros(0, np.float32)
    return _pack(off, cat(mzs), cat(ints))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class _Edges:
    """The edge fixture as a batch, with the kernel's and the oracle's features of it (computed
    once, read by every test)."""

    def __init__(self, O):
        from ann_solo_amd import spectrum_similarity as sim
        self.E = E = EdgeCases()
        self.F = sim.ssm_features(*self.batch(range(E.n)))
        self.F.setflags(write=False)
        self.want = np.stack([O.ssm_features(*E.case(c)) for c in range(E.n)])
        self.want.setflags(write=False)

    def batch(self, sel, stride=None):
        """(Q, L, lib_rows, pairs, counts) of the fixture cases `sel`, in that order."""
        E, sel = self.E, list(sel)
        cs = [E.case(c) for c in sel]
        pairs, cnt = E.pairs(sel, stride)
        return (_pack_list([c[0] for c in cs], [c[1] for c in cs]),
                _pack_list([c[2] for c in cs], [c[3] for c in cs]),
                np.arange(len(sel), dtype=np.int32), pairs, cnt)


@pytest.fixture(scope='module')
def edges(O):
    return _Edges(O)


def _deviation(got, want):
    """|got - want| in units of the oracle bound, per column (0 where both are the same inf)."""
    with np.errstate(invalid='ignore'):
        d = np.abs(got - want) / (1e-11 + 1e-9 * np.abs(want))
    return np.where(got == want, 0.0, d)


def test_edge_fixture_parity(O, edges):
    """The whole fixture in one batch: every case against the reference's values and against the
    oracle, inf columns exactly inf (check_features compares non-finite values with ==), and
    the `*_top` columns with top = 1, 3, 12 passed through."""
    from ann_solo_amd import spectrum_similarity as sim
    E, F = edges.E, edges.F
    assert F.shape == (E.n, sim.N_FEATURES)
    dev = _deviation(F, edges.want)
    print('deviation from the oracle / bound, max per column:',
          ' '.join('%d:%.3g' % (f, dev[:, f].max()) for f in range(F.shape[1])))
    print('worst case per column:', ' '.join('%d:%s' % (f, E.names[int(dev[:, f].argmax())])
                                             for f in range(F.shape[1]) if dev[:, f].max() > 0.01))
    for c in range(E.n):
        check_features(F[c], E.features[c], f'reference {E.names[c]}')
        check_features(F[c], edges.want[c], f'oracle {E.names[c]}', **ORACLE_TOL)
    assert np.isinf(E.features).sum() > 0
    assert np.array_equal(np.isinf(F), np.isinf(E.features)) and (F[np.isinf(F)] > 0).all()
    Q, L, rows, pairs, cnt = edges.batch(range(E.n))
    for ti, t in enumerate(E.tops):
        Ft = sim.ssm_features(Q, L, rows, pairs, cnt, top=t)
        want_t = np.stack([O.ssm_features(*E.case(c), top=t) for c in range(E.n)])
        print(f'top={t}: deviation from the oracle / bound, max per top column:',
              ' '.join('%d:%.3g' % (f, _deviation(Ft, want_t)[:, f].max()) for f in E.top_columns))
        for c in range(E.n):
            if E.nl[c] >= 13:
                check_top_features(Ft[c], E.features_top[c, ti], E.top_columns,
                                   f'reference {E.names[c]} top={t}')
            check_features(Ft[c], want_t[c], f'oracle {E.names[c]} top={t}', **ORACLE_TOL)


def test_both_instantiations_give_the_same_bits(edges):
    """The SSMs of at most 128 peaks alone (the 128-peak kernel) and inside the full batch (the
    wide cases force the 256-peak re-launch of all of it): the same rows as uint64."""
    from ann_solo_amd import spectrum_similarity as sim
    E = edges.E
    narrow = [c for c in range(E.n) if E.nq[c] <= 128 and E.nl[c] <= 128]
    assert 20 <= len(narrow) < E.n and max(E.cnt[narrow]) == 120
    Fn = sim.ssm_features(*edges.batch(narrow))
    assert np.array_equal(_bits(Fn), _bits(edges.F[narrow]))


def test_batch_structure(edges):
    """An odd batch (the last workgroup has an idle wave), rows without a library spectrum (-1)
    and one beyond the library, in fixture order and permuted, host and device inputs."""
    import torch
    from ann_solo_amd import spectrum_similarity as sim
    E = edges.E
    sel = list(range(E.n)) + [0]
    n = len(sel)
    assert n % 2 == 1
    Q, L, rows, pairs, cnt = edges.batch(sel)
    rows[2::3] = -1
    rows[4] = L.n + 5
    gone = np.zeros(n, bool)
    gone[2::3] = gone[4] = True
    Fa = sim.ssm_features(Q, L, rows, pairs, cnt)
    assert np.isnan(Fa[gone]).all() and not np.isnan(Fa[~gone]).all(1).any()
    assert np.array_equal(_bits(Fa[~gone]), _bits(edges.F[np.array(sel)[~gone]]))
    perm = np.random.default_rng(5).permutation(n)
    Qp = edges.batch([sel[k] for k in perm])[0]
    Fp = sim.ssm_features(Qp, L, rows[perm], pairs[perm], cnt[perm])
    assert np.array_equal(_bits(Fp), _bits(Fa[perm]))
    dev = lambda a: torch.from_numpy(a).cuda()
    Fd = sim.ssm_features(Qp.to('cuda'), L.to('cuda'), dev(rows[perm]),
                          dev(pairs[perm].view(np.int32)), dev(cnt[perm]))
    assert np.array_equal(_bits(Fd.cpu().numpy()), _bits(Fp))


def test_cosine_kernel_on_the_edge_batch(edges):
    """ssm_cosine == column 0 bit for bit, the 100- and 200-match cases included (its
    lane-strided accumulation wraps there)."""
    from ann_solo_amd import spectrum_similarity as sim
    c0 = sim.ssm_cosine(*edges.batch(range(edges.E.n)))
    assert np.array_equal(_bits(c0), _bits(edges.F[:, 0]))


def test_values_only_the_oracle_defines(O):
    """A library shorter than `top`, one match, no match behind a valid row, and empty spectra
    behind a valid row: the reference raises or never sees these; the kernel gives the
    oracle's values and the closed forms tests/test_oracle_similarity.py asserts of it."""
    from ann_solo_amd import spectrum_similarity as sim
    mz = np.linspace(100, 1000, 12).astype(np.float32)
    it = (np.arange(12) + 1).astype(np.float32)
    it /= np.linalg.norm(it)
    e = np.zeros(0, np.float32)
    unit = lambda v: v / np.linalg.norm(v)
    three = [[0, 0], [2, 1], [5, 2]]
    ssms = [('nl=3', mz, it, mz[:3], unit(it[:3]), three),
            ('nl=4', mz, it, mz[:4], unit(it[:4]), three),
            ('one match', mz, it, mz, it, [[3, 3]]),
            ('no match', mz, it, mz, it, []),
            ('empty query', e, e, mz, it, []),
            ('empty library', mz, it, e, e, []),
            ('both empty', e, e, e, e, [])]
    pairs = np.zeros((len(ssms), 3, 2), np.uint32)
    cnt = np.array([len(s[5]) for s in ssms], np.int32)
    for i, s in enumerate(ssms):
        pairs[i, :cnt[i]] = np.asarray(s[5], np.uint32).reshape(-1, 2)
    F = sim.ssm_features(_pack_list([s[1] for s in ssms], [s[2] for s in ssms]),
                         _pack_list([s[3] for s in ssms], [s[4] for s in ssms]),
                         np.arange(len(ssms), dtype=np.int32), pairs, cnt)
    for i, (tag, q_mz, q_int, l_mz, l_int, pm) in enumerate(ssms):
        want = O.ssm_features(q_mz, q_int, l_mz, l_int, np.asarray(pm, np.uint32).reshape(-1, 2))
        assert not np.isnan(want).any()
        check_features(F[i], want, tag, **ORACLE_TOL)
        if not pm:
            closed = want.copy()
            closed[list(NO_MATCH)] = list(NO_MATCH.values())
            check_features(F[i], closed, tag + ' closed form', **ORACLE_TOL)
            if not len(l_mz):
                assert F[i][15] == 100.0
    for i, nl in ((0, 3), (1, 4)):
        f = F[i]
        assert np.isfinite(f).all() and f[2] == 3
        assert f[4] == pytest.approx(3 / nl, rel=1e-12) and f[5] == pytest.approx(3 / nl, rel=1e-12)
        for top_col, col in ((8, 7), (10, 9), (12, 11), (22, 21), (27, 26), (29, 28)):
            assert f[top_col] == f[col], (nl, top_col)
    assert F[2][2] == 1 and F[2][16] == 0.0 and F[2][0] == pytest.approx(float(it[3]) ** 2, rel=1e-6)


def test_peak_match_counts(O, edges):
    """include/annsolo_mi.h's rule for pm_count: clipped to pm_stride; negative = invalid, from
    both entries; up to 256 pairs (a list that repeats peaks, no matching has that many on 50
    peaks) are answered by the wide kernel, more is the capacity error. The valid rows beside a
    count that is handled keep the bits they have alone; where the call raises, the batch
    without the bad row does."""
    from ann_solo_amd import _lib
    from ann_solo_amd import spectrum_similarity as sim
    E = edges.E
    # (a) above the stride = the stride
    sel = [c for c in range(E.n) if E.cnt[c] >= 20][:9]
    Q, L, rows, pairs, cnt = edges.batch(sel)
    pairs = np.ascontiguousarray(pairs[:, :10])
    ten = np.full(len(sel), 10, np.int32)
    over = cnt.copy()
    over[::2] = 2 ** 31 - 1
    assert (over > 10).all()
    F10 = sim.ssm_features(Q, L, rows, pairs, ten)
    assert np.isfinite(F10[:, 0]).all() and (F10[:, 2] == 10).all()
    assert np.array_equal(_bits(sim.ssm_features(Q, L, rows, pairs, over)), _bits(F10))
    assert np.array_equal(_bits(sim.ssm_cosine(Q, L, rows, pairs, over)), _bits(F10[:, 0]))
    # (b) negative
    for bad_value in (-1, -2 ** 31):
        neg = ten.copy()
        neg[3] = bad_value
        with pytest.raises(_lib.AnnSoloMiError, match='negative'):
            sim.ssm_features(Q, L, rows, pairs, neg)
        with pytest.raises(_lib.AnnSoloMiError, match='negative'):
            sim.ssm_cosine(Q, L, rows, pairs, neg)
    rows_wo = rows.copy()
    rows_wo[3] = -1                        # the same batch without the bad row
    keep = rows_wo >= 0
    assert np.array_equal(_bits(sim.ssm_features(Q, L, rows_wo, pairs, ten)[keep]), _bits(F10[keep]))
    assert np.array_equal(_bits(sim.ssm_cosine(Q, L, rows_wo, pairs, ten)[keep]), _bits(F10[keep, 0]))
    # (c) 129 .. 256 pairs on 50-peak spectra
    rng = np.random.default_rng(11)
    mzs = [np.sort(rng.uniform(100, 1900, 50)).astype(np.float32) for _ in range(4)]
    ints = [(lambda v: (v / np.linalg.norm(v)).astype(np.float32))(rng.permutation(50) + 1.0 + 0.5 * k)
            for k in range(4)]
    P = _pack_list(mzs, ints)
    lib_rows = np.array([1, 0, 3, 2], np.int32)
    full = np.stack([np.arange(50), rng.permutation(50)], 1)       # a matching of all 50 peaks
    part = np.stack([np.sort(rng.choice(50, 10, replace=False)),
                     rng.choice(50, 10, replace=False)], 1)        # ... and of 10 of them
    lists = [full[:20], full[np.arange(200) % 50], part[np.arange(130) % 10], full[np.arange(256) % 50]]

    def padded(ls, stride):
        out = np.zeros((len(ls), stride, 2), np.uint32)
        for i, l in enumerate(ls):
            out[i, :len(l)] = l
        return out, np.array([len(l) for l in ls], np.int32)
    pp, pc = padded(lists, 256)
    Fw = sim.ssm_features(P, P, lib_rows, pp, pc)
    for i, l in enumerate(lists):
        r = lib_rows[i]
        want = O.ssm_features(mzs[i], ints[i], mzs[r], ints[r], l)
        check_features(Fw[i], want, f'{len(l)} pairs', **ORACLE_TOL)
    assert list(Fw[:, 2]) == [20, 200, 130, 256]
    alone = sim.ssm_features(P, P, np.array([1, -1, -1, -1], np.int32), pp, pc)   # 128-peak kernel
    assert np.array_equal(_bits(alone[0]), _bits(Fw[0])) and np.isnan(alone[1:]).all()
    assert np.array_equal(_bits(sim.ssm_cosine(P, P, lib_rows, pp, pc)), _bits(Fw[:, 0]))
    # (d) beyond the capacity: 257 pairs, and 256 pairs that leave 40 library peaks unmatched
    for too_long in (full[np.arange(257) % 50], part[np.arange(256) % 10]):
        pp, pc = padded([lists[0], lists[1], too_long, lists[3]], 257)
        with pytest.raises(_lib.AnnSoloMiError, match='pairs'):
            sim.ssm_features(P, P, lib_rows, pp, pc)
        rows_wo = lib_rows.copy()
        rows_wo[2] = -1
        Fr = sim.ssm_features(P, P, rows_wo, pp, pc)
        assert np.array_equal(_bits(Fr[[0, 1, 3]]), _bits(Fw[[0, 1, 3]])) and np.isnan(Fr[2]).all()
