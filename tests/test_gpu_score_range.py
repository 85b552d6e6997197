"""The fused top-k of every list scan on scores OUTSIDE the histogram's range (csrc/hist_topk.hpp buckets
[-0.25, 1); "scores outside clamp to the end buckets, which only costs resolution there, never exactness") and
on thousands of DISTINCT scores inside one bucket (the exact sort-and-truncate fallback entered without a
single duplicate): ids and score bits of every search form against the oracle, on the regimes of
tests/score_range_cases.py (whose properties tests/test_score_range_cases_cpu.py holds). Every comparison is
bit for bit: a regime is the control scaled by a power of two or with signs changed, so the oracle's chain
and the kernels' still compute the same numbers."""
import numpy as np
import pytest

import raw_pq_ref as R
import score_range_cases as S

pytestmark = pytest.mark.gpu

K_REF = max(S.KS)            # one oracle search per (regime, form, nprobe); a smaller k is its leading columns


@pytest.fixture(scope='module')
def world(O):
    """name -> the oracle's side of a regime (built on first use), with its reference rows cached."""
    cache = {}

    def get(name):
        if name not in cache:
            h = S.host_indexes(O, name)
            h['fx22'] = O.HostIVF(h['cen'], h['assign'], O.quantize_fx22(h['xb']))
            h['rows'] = {}
            cache[name] = h
        return cache[name]
    return get


def ref_rows(O, h, form, nprobe, k):
    """The oracle's (D, I) [nq, k] of one search form: 'brute' | 'flat' | 'fx22' | 'pq' | 'raw'."""
    key = (form, nprobe)
    if key not in h['rows']:
        if form == 'brute':
            h['rows'][key] = O.flat_search(h['xb'], h['xq'], K_REF)
        elif form == 'raw':
            h['rows'][key] = R.raw_search(O, h['xq'], h['cen'], h['raw'], K_REF, nprobe)
        else:
            h['rows'][key] = h[form].search(h['xq'], K_REF, nprobe)
        h['rows'][key][0].setflags(write=False)
        h['rows'][key][1].setflags(write=False)
    Dr, Ir = h['rows'][key]
    return Dr[:, :k], Ir[:, :k]


def assert_rows(got, want, what):
    (D, I), (Do, Io) = got, want
    assert np.array_equal(I, Io), what
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what


def assert_same_sets(got, want, what):
    """Unordered rows: the oracle's ids with the oracle's score bits in any order, padding last."""
    (D, I), (Do, Io) = got, want
    for r in range(len(Io)):
        n = int((Io[r] >= 0).sum())
        assert (I[r, :n] >= 0).all() and (I[r, n:] == -1).all(), (what, r)
        o, oo = np.argsort(I[r, :n]), np.argsort(Io[r, :n])
        assert np.array_equal(I[r, :n][o], Io[r, :n][oo]), (what, r)
        assert np.array_equal(D[r, :n][o].view(np.uint32), Do[r, :n][oo].view(np.uint32)), (what, r)


def unpack_keys(K):
    """Packed hits (ord(score) << 32 | ~id, 0 = empty) -> (score bits uint32, ids int64 with -1)."""
    K = K.view(np.uint64)
    ids = np.where(K != 0, 0xFFFFFFFF - (K & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    ordb = (K >> np.uint64(32)).astype(np.uint32)
    bits = np.where(ordb & 0x80000000, ordb & 0x7fffffff, ~ordb).astype(np.uint32)      # ord2f
    return bits, ids


def assert_keys(K, want, what):
    bits, ids = unpack_keys(K)
    Do, Io = want
    for r in range(len(Io)):
        n = int((Io[r] >= 0).sum())
        assert int((ids[r] >= 0).sum()) == n, (what, r)
        o = np.argsort(np.where(ids[r] >= 0, ids[r], 1 << 40))[:n]
        oo = np.argsort(Io[r, :n])
        assert np.array_equal(ids[r][o], Io[r, :n][oo]), (what, r)
        assert np.array_equal(bits[r][o], Do[r, :n][oo].view(np.uint32)), (what, r)


def probes(h):
    return (h['nlist'], 2)


def check_ivf(O, idx, h, form, variants, expect_keys=True):
    """Every k and nprobe of the module on one IVF index: ordered rows under each scan variant, then -- on the
    layout-specific scan -- the unordered rows as sets and the packed-key rows where the index emits them."""
    from ann_solo_amd import _lib
    L = _lib.lib()
    xq = h['xq']
    for variant in variants:
        idx.set_scan_variant(variant)
        for nprobe in probes(h):
            idx.nprobe = nprobe
            for k in S.KS:
                assert_rows(idx.search(xq, k), ref_rows(O, h, form, nprobe, k), (h['name'], form, variant, k, nprobe))
    idx.set_scan_variant(0)
    n_keys = 0
    for nprobe in probes(h):
        idx.nprobe = nprobe
        cD, cI = idx.coarse(xq, nprobe)
        for k in S.KS:
            want = ref_rows(O, h, form, nprobe, k)
            idx.set_unordered(1)
            try:
                got = idx.search(xq, k)
            finally:
                idx.set_unordered(0)
            assert_same_sets(got, want, (h['name'], form, 'unordered', k, nprobe))
            if L.asl_index_supports_keys(idx._h, k, nprobe) == 1:
                n_keys += 1
                assert_keys(idx.search_preassigned_keys(xq, k, cD, cI), want, (h['name'], form, 'keys', k, nprobe))
    if expect_keys:          # the sparse layouts emit keys at every k <= 1280
        assert n_keys >= 2 * sum(1 for k in S.KS if k <= 1280)
    assert_rows(idx.search(xq, 100), ref_rows(O, h, form, idx.nprobe, 100), 'the modes do not stick')


def same_lists(idx, ivf):
    off, ids, payload = idx.lists()
    return (np.array_equal(off, ivf.list_offsets) and np.array_equal(ids, ivf.ids) and
            np.array_equal(payload, ivf.payload))


@pytest.mark.parametrize('name', S.REGIMES)
def test_flat_ip_rows(O, world, name):
    """IndexFlatIP: `row_topk_kernel` over all 6 000 rows at every k (k = 2 500 in bounded passes), and
    `row_select_kernel` -- a histogram over the row's own [min, max] -- over the first 4 096 and 1 000 rows at
    k <= 256."""
    from ann_solo_amd import faiss_compat as faiss
    h = world(name)
    idx = faiss.IndexFlatIP(S.D)
    idx.add(h['xb'])
    for k in S.KS:
        assert_rows(idx.search(h['xq'], k), ref_rows(O, h, 'brute', 0, k), (name, k))
    for n in (4096, 1000):
        sub = faiss.IndexFlatIP(S.D)
        sub.add(h['xb'][:n])
        for k in (1, 100, 256):
            assert_rows(sub.search(h['xq'], k), O.flat_search(h['xb'][:n], h['xq'], k), (name, n, k))


@pytest.mark.parametrize('name,storage', [(n, 'fp32') for n in S.REGIMES] + [(n, 'fx22') for n in S.FX22_REGIMES])
def test_ivfflat_rows(O, world, name, storage):
    """IndexIVFFlat: the postings scan (variant 0, both key-buffer sizes: k <= 1 280 and beyond) and the
    generic kernels (variant 1); `wide_lists` probes 600 lists, two per thread. 'fx22' on the regimes whose
    components lie in [0, 1) -- on `tiny` every stored component rounds to 0: no postings, every score ties."""
    from ann_solo_amd import faiss_compat as faiss
    h = world(name)
    form = 'flat' if storage == 'fp32' else 'fx22'
    idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(S.D), S.D, h['nlist'], storage=storage)
    idx.set_trained(h['cen'])
    idx.add(h['xb'])
    all_zero = storage == 'fx22' and name == 'tiny'
    assert idx.flat_layout == (1 if storage == 'fp32' else 0 if all_zero else 2)
    assert same_lists(idx, h[form]) and (np.count_nonzero(h[form].payload) == 0) == all_zero
    check_ivf(O, idx, h, form, (0, 1), expect_keys=not all_zero)


@pytest.mark.parametrize('by_residual', [True, False])
@pytest.mark.parametrize('name', S.REGIMES)
def test_ivfpq_rows(O, world, name, by_residual):
    """IndexIVFPQ, m = 32, 8 bits: the tiled scan from the sub-quantiser-major codes (variant 0), from the
    tile-major codes only (variant 2) and the generic `pq_scan_kernel` (variant 1), coding residuals and coding
    the vectors themselves."""
    from ann_solo_amd import faiss_compat as faiss
    h = world(name)
    form = 'pq' if by_residual else 'raw'
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(S.D), S.D, h['nlist'], S.PQ_M, 8)
    if not by_residual:
        idx.by_residual = False
    idx.set_trained(h['cen'], h['cb'] if by_residual else h['raw_cb'])
    idx.add(h['xb'])
    assert same_lists(idx, h[form])
    check_ivf(O, idx, h, form, (0, 2, 1))


@pytest.mark.parametrize('name', ['above_one', 'negated'])
def test_refined_rows(O, world, name):
    """`set_refine(1024)`, k = 256: the ADC scan's 1 024 best -- all of them in an end bucket -- re-ranked with
    the exact inner product, against `O.refine` of the oracle's short-list."""
    from ann_solo_amd import faiss_compat as faiss
    h = world(name)
    idx = faiss.IndexIVFPQ(faiss.IndexFlatIP(S.D), S.D, h['nlist'], S.PQ_M, 8)
    idx.set_refine(1024)
    idx.set_trained(h['cen'], h['cb'])
    idx.add(h['xb'])
    for nprobe in probes(h):
        idx.nprobe = nprobe
        _, I_short = ref_rows(O, h, 'pq', nprobe, 1024)
        assert_rows(idx.search(h['xq'], 256), O.refine(h['xb'], h['xq'], I_short, 256), (name, nprobe))


@pytest.mark.parametrize('kind', ['pq', 'flat'])
@pytest.mark.parametrize('name', ['above_one', 'far_below', 'one_bucket', 'across_one'])
def test_three_shards_merge_to_the_oracles_rows(O, world, name, kind):
    """A three-way split on one GPU merged by `asl_topk_merge`: `topk_merge_hist_kernel` at both of its
    capacities (k = 1 024: 2 048 keys; k = 2 048: 4 096 keys), fed scores that all clamp to one end bucket,
    crowd one interior bucket or lie on both sides of 1; against the UNSHARDED oracle rows."""
    from ann_solo_amd import faiss_compat as faiss
    h = world(name)

    def make():
        if kind == 'pq':
            ix = faiss.IndexIVFPQ(faiss.IndexFlatIP(S.D), S.D, h['nlist'], S.PQ_M, 8)
            ix.set_trained(h['cen'], h['cb'])
        else:
            ix = faiss.IndexIVFFlat(faiss.IndexFlatIP(S.D), S.D, h['nlist'])
            ix.set_trained(h['cen'])
        ix.add(h['xb'])
        ix.nprobe = h['nlist']
        return ix
    shards = []
    for r in range(3):
        sh = make()
        sh.shard(r, 3)
        assert sh.ntotal == S.N
        shards.append(sh)
    assert sum(sh.info().nlocal for sh in shards) == S.N
    for k in (1024, 2048):
        parts = [sh.search(h['xq'], k) for sh in shards]
        Ds, Is = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        want = ref_rows(O, h, kind, h['nlist'], k)
        assert_rows(faiss.topk_merge(Ds, Is), want, (name, kind, k))
        assert_rows(O.topk_merge(Ds, Is), want, (name, kind, k, 'oracle merge'))


def _select_rows(case, n, rng):
    """(xb [n, 2], xq [nq, 2]) whose score rows stress `scale = 511 / (hi - lo)` of `row_select_kernel`."""
    xb = np.zeros((n, 2), np.float32)
    if case == 'constant':                       # hi == lo at a non-zero value
        xb[:, 0] = 3.5
        xq = np.array([[1, 0], [2, 5], [-1, 0]], np.float32)
    elif case == 'ulps':                         # 37 +- a few ulps: hi - lo is a handful of ulps of a large value
        base = np.float32(37.0).view(np.int32)
        xb[:, 0] = (base + rng.integers(-3, 4, n).astype(np.int32)).view(np.float32)
        xq = np.array([[1, 0], [-1, 0], [1, 9]], np.float32)
    else:                                        # hi - lo overflows fp32, every score stays finite
        xb[:, 0] = (rng.choice([-1.0, 1.0], n) * (0.5 + 0.5 * rng.random(n)) * 1.8e19).astype(np.float32)
        xb[:, 1] = rng.standard_normal(n).astype(np.float32)
        xq = np.array([[1.8e19, 0], [-1.8e19, 1], [1.8e19, -3]], np.float32)
    return xb, xq


@pytest.mark.parametrize('n', [100, 4096])
@pytest.mark.parametrize('case', ['constant', 'ulps', 'overflow'])
def test_row_select_on_degenerate_ranges(O, case, n):
    """`row_select_kernel` buckets a short row over its own [min, max]: a constant non-zero row, a spread of a
    few ulps around 37, and a row whose `hi - lo` is infinite in fp32 while every score is finite; k > n pads
    with -1. No infinity and no NaN anywhere."""
    from ann_solo_amd import faiss_compat as faiss
    xb, xq = _select_rows(case, n, np.random.default_rng(n + len(case)))
    idx = faiss.IndexFlatIP(2)
    idx.add(xb)
    for k in (1, 7, 256):
        Do, Io = O.flat_search(xb, xq, k)
        valid = Io >= 0
        assert np.isfinite(Do[valid]).all() and valid.sum() == len(xq) * min(k, n)
        if k == 256:             # the whole row of the first query, not its k best
            row = O.flat_search(xb, xq[:1], n)[0][0]
            hi, lo = row.max(), row.min()
            with np.errstate(over='ignore'):
                spread = np.float32(hi) - np.float32(lo)
            assert {'constant': spread == 0 and hi != 0, 'ulps': 0 < spread < 1e-4,
                    'overflow': np.isinf(spread)}[case], (case, lo, hi)
        D, I = idx.search(xq, k)
        assert np.array_equal(I, Io), (case, n, k)
        assert np.array_equal(D.view(np.uint32)[valid], Do.view(np.uint32)[valid]), (case, n, k)
        assert (I[:, n:] == -1).all()
