"""The batch-shape cases (tests/batch_cases.py) really reach the decisions that
tests/test_gpu_batch_shapes.py is there to pin: the pools hold the rows they claim, the batches fall on
both sides of every batch-derived threshold, the periodic queries cannot line up with a chunk. Each rule
of the product is restated in one line (in batch_cases.py, with its source line) and applied to the cases.
Without this the GPU tests could pass by never leaving the comfortable path."""
import math

import numpy as np

import batch_cases as BC


def test_coarse_pool_holds_what_it_claims():
    x, dense = BC.coarse_pool()
    nnz = np.count_nonzero(x, axis=1)
    assert x.shape == (96, BC.COARSE_D) and nnz[0] == 0
    assert (nnz[:72] <= 50).all() and (nnz[72:80] == 64).all()
    assert (nnz[80:] >= 65).all() and (nnz[80:] <= 90).all()
    assert int(dense.sum()) == 16 and dense[80:].all()          # 64 non-zeros still fit the registers
    assert (x < 0).any() and len(set(nnz[:72].tolist())) > 20
    for nlist in BC.COARSE_NLISTS:
        cen = BC.coarse_centroids(nlist)
        cn = np.count_nonzero(cen, axis=1)
        assert cen.shape == (nlist, BC.COARSE_D) and cn.min() >= 8 and cn.max() <= 200 and (cen < 0).any()


def test_coarse_cases_cover_both_sides_of_the_gate():
    _, dense = BC.coarse_pool()
    batches = BC.coarse_batches(dense)
    assert [(m, n) for m, n, _ in batches] == list(BC.COARSE_CASES)
    # the rule (csrc/index_search.hip:26 `over_max = m / 64`; csrc/coarse_sparse.hip:112 `if (*n_over > over_max) return;`)
    gemm = lambda m, n_over: n_over > m // 64
    outcome = {}
    for m, n_dense, take in batches:
        assert len(take) == m and int(dense[take].sum()) == n_dense
        assert BC.gemm_takes_the_batch(m, n_dense) == gemm(m, n_dense)
        outcome.setdefault(m, {})[n_dense] = gemm(m, n_dense)
    # n_over at over_max (the sparse kernel keeps the batch) and at over_max + 1 (the GEMM takes it)
    for m in (1, 63, 64, 127, 128, 129, 257):
        assert outcome[m][m // 64] is False and outcome[m][m // 64 + 1] is True, m
    assert outcome[65] == {1: False} and outcome[2] == {1: True}
    # a dense row first, last and in the middle
    at = {(m, tuple(np.nonzero(dense[take])[0])) for m, _, take in batches}
    assert any(p == (0,) for _, p in at) and any(len(p) == 1 and p[0] == m - 1 and m > 1 for m, p in at)
    assert any(len(p) == 1 and p[0] == m // 2 and 0 < m // 2 < m - 1 for m, p in at)
    # partial groups of 4 rows (list_nonzeros_kernel, the sparse kernel's wave) and of 64 (a workgroup pass)
    assert {m % 4 for m, _ in BC.COARSE_CASES} == {0, 1, 2, 3} and {63, 64, 65} <= {m for m, _ in BC.COARSE_CASES}


def test_index_pool_and_batches(O):
    xb, pool, dense = BC.index_vectors(O)
    assert xb.shape == (BC.INDEX_N, 800) and pool.shape == (72, 800)
    nnz = np.count_nonzero(pool, axis=1)
    assert (nnz[:64] <= 50).all() and (nnz[64:] > 64).all() and int(dense.sum()) == 8
    assert xb.min() >= 0.0 and xb.max() < 1.0                      # fixed-point storage takes them
    batches = BC.index_batches(dense)
    assert sorted({s for s, _, _ in batches}) == sorted(BC.INDEX_SIZES) and len(batches) == 2 * len(BC.INDEX_SIZES)
    gemm = {}
    for size, draw, take in batches:
        assert len(take) == size and take.min() >= 0 and take.max() < 72
        n_over = int(dense[take].sum())
        if size >= 63 and draw == 0:
            assert n_over >= 1
        if draw == 1:
            assert n_over == size // 64
        gemm.setdefault(size, set()).add(BC.gemm_takes_the_batch(size, n_over))
    for size in BC.INDEX_SIZES:                                    # the gate flips inside search as well
        if size >= 63:
            assert gemm[size] == {True, False}, size
    assert any(len(set(take.tolist())) < len(take) for _, _, take in batches)      # an item meets itself


def test_periodic_queries_cannot_line_up_with_a_chunk():
    assert BC.chunk_rows(BC.CHUNK_N) == 1024 and BC.chunk_rows(BC.CLOOP['nlist']) == 65536
    for rows in (1024, 65536):
        assert math.gcd(BC.CHUNK_POOL, rows) == 1
    # every case reaches a second chunk; 1025 and 65537 end on a chunk of one row, 2049 has three chunks
    for nq, _ in BC.CHUNK_FLAT:
        assert nq > 1024
    assert BC.CHUNK_IVF['nq'] == 1025 and 2049 == 2 * 1024 + 1 and BC.CLOOP['nq'] == 65536 + 1
    assert any(k > 2048 for _, k in BC.CHUNK_FLAT)                 # TK_MAX_K: the bounded second pass
    pool = np.arange(BC.CHUNK_POOL, dtype=np.float32)[:, None]
    xq = BC.periodic(pool, 1025)
    assert xq[1024, 0] == 1024 % 37 != xq[0, 0]                    # row 0 of chunk 1 is not row 0 of chunk 0
    # postings need sparse vectors: the most non-zeros of a vector, times 8, below d
    assert BC.CLOOP['nnz'] * 8 < BC.CLOOP['d']
    cen, xb, qp = BC.cloop_vectors()
    assert (np.count_nonzero(xb, axis=1) == 4).all() and (np.count_nonzero(cen, axis=1) == 4).all()
    assert qp.shape == (37, 64)


def test_rescore_cases_reach_their_split(O):
    from score_hist_ref import pair_scores
    lib, pool = BC.rescore_spectra()
    ln, qn = np.diff(lib[0]), np.diff(pool[0])
    assert len(ln) == 64 and len(qn) == 4
    assert ((ln[40:52] >= 65) & (ln[40:52] <= 150)).all() and ln[:40].max() <= 64 and ln[52:].max() <= 64
    assert qn.max() > 100 and np.sort(qn)[-2] <= 100
    for o, mz in ((lib[0], lib[1]), (pool[0], pool[1])):
        for i in range(len(o) - 1):
            assert np.all(np.diff(mz[o[i]:o[i + 1]]) > 0)
    for r in range(52, 64):                                        # a twin half a tolerance above its peak
        gaps = np.diff(lib[1][lib[0][r]:lib[0][r + 1]].astype(np.float64))
        assert abs(gaps.min() - BC.RS_TOL / 2) < 1e-3
    Q, L = O.Spectra(*pool), O.Spectra(*lib)
    for tol in (BC.RS_TOL, 0.0):
        S = np.stack([pair_scores(O, Q, q, L, np.arange(64), tol, True) for q in range(4)])
        assert (S >= 0).all() and (S.max(axis=1) > 0).all()
        # the rule (csrc/rescore.hip:1609-1611, rescore_device: avg = total_slots / nq, split when nq < 2048 && avg > 4096)
        rule = lambda nq, total: min(64, -(-(total // nq) // 4096)) if nq < 2048 and total // nq > 4096 else 1
        reached = []
        for ci, (nq, lens) in enumerate(BC.RS_CASES):
            if tol == 0.0 and ci not in BC.RS_TOL0_CASES:
                reached.append(BC.RS_YSPLIT[ci])
                continue
            item, rows, off = BC.rescore_case(ci, S)
            assert len(item) == nq and len(off) == nq + 1 and off[-1] == len(rows)
            ys = rule(nq, int(off[-1]))
            assert ys == BC.ysplit(nq, int(off[-1]))
            reached.append(ys)
            for q in range(nq):
                c = rows[off[q]:off[q + 1]]
                if len(c):                                        # every non-empty list has a positive maximum
                    assert S[item[q], c].max() > 0
            if ys > 1:
                c = rows[off[0]:off[1]]
                top = np.nonzero(S[item[0], c] == S[item[0], c].max())[0]
                assert top.tolist() == [40, 64 * ys + 3, len(c) - 1]
                # groups of 32 slots of a 1024-slot super-chunk go to the blocks round robin: slot 40 is another
                # block's than slot 64 * ysplit + 3, which is block 0's
                assert ((40 % 1024) >> 5) % ys != 0 and (((64 * ys + 3) % 1024) >> 5) % ys == 0
            assert len(set(rows[:off[1]].tolist())) < off[1]       # rows repeat
        assert tuple(reached) == BC.RS_YSPLIT
    assert BC.ysplit(1, 258048) == 63 and BC.ysplit(2048, 2048 * 300000) == 1


def test_encoder_pool_and_batches():
    o, mz, it = BC.encoder_pool()
    n = np.diff(o)
    assert len(n) == BC.ENC_POOL and tuple(n[:7]) == BC.ENC_SIZES and len(mz) == len(it) == o[-1]
    for i in range(1, BC.ENC_POOL):                                # colliding bins: an m/z repeats
        if 2 < n[i] <= 100:
            assert len(np.unique(mz[o[i]:o[i + 1]])) < n[i]
    batches = BC.encoder_batches()
    assert sorted({len(b) for b in batches}) == list(BC.ENC_BATCHES)
    assert {len(b) % 4 for b in batches} == {0, 1, 2, 3}            # ENC_WAVES = 4 spectra per workgroup
    seen = set(np.concatenate(batches).tolist())
    assert {0, 1, 2, 3, 4, 5, 6} <= seen                           # empty, 1, 2, 63, 64, 65, 200 peaks
    off, bm, bi = BC.gather_peaks((o, mz, it), batches[-1])
    assert off[-1] == len(bm) == len(bi) == int(n[batches[-1]].sum())
