"""Every compiled form of the IVF-Flat postings scan (csrc/flat_scan.hip: flat_inv_scan picks one of the 14
instantiations of flat_inv_scan_kernel<CAP, FX, WIDE, SEL, RANGED>) against the oracle's ``HostIVF.search``: ids
equal, scores equal bit for bit. A request routed to the wrong form either fails here or, where the wrong form
happens to compute the same rows, is caught by what decides the form: the index's reported layout (FX) and the
shape rules of the dispatcher (WIDE: more than 512 probes; CAP: k + 768 <= 2048 keys or 4096).

One small library per storage, shared by the cases: d = 130 with at most 16 non-zeros per vector (the postings
are built while 8 * nnz_max < d), 520 lists so that nprobe is 8 (one probe per thread) or 520 (WIDE), four of them
longer than one block of 832 vectors; k = 64 (2048 keys) or 1300 (the smallest k of the 4096-key region)."""
import numpy as np
import pytest

import selector_ref as R
import winflat_ref as WR

pytestmark = pytest.mark.gpu

FI_BLK, FI_NT = 832, 512               # csrc/flat_postings.hpp, csrc/flat_scan.hip
D, NNZ, N, NLIST, NQ = 130, 16, 6000, 520, 16
HEAVY, SHARED = 4, 12                  # four prototypes, each sharing its 12 dimensions with 1200 vectors

# (CAP, FX, WIDE, SEL, RANGED): what flat_scan.hip instantiates -- plain requests at both key capacities, the
# selector and the ranged form (the window-exact index: one list, no probes) at 2048 keys only
FORMS = ([(cap, fx, wide, False, False) for cap in (2048, 4096) for fx in (False, True) for wide in (False, True)] +
         [(2048, fx, wide, True, False) for fx in (False, True) for wide in (False, True)] +
         [(2048, fx, False, False, True) for fx in (False, True)])
assert len(FORMS) == 14 and len(set(FORMS)) == 14


def _rows(rng, n, proto):
    """n unit vectors of NNZ non-zeros; row i < HEAVY * 1200 shares SHARED dimensions with prototype i % HEAVY."""
    x = np.zeros((n, D), np.float32)
    for i in range(n):
        cols = rng.choice(D, NNZ, replace=False)
        if i < HEAVY * 1200:
            cols[:SHARED] = proto[i % HEAVY]                     # (a repeated column: fewer non-zeros)
        x[i, cols] = rng.random(NNZ, dtype=np.float32) * 0.9 + 0.05
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.fixture(scope='module')
def library():
    rng = np.random.default_rng(20260130)
    proto = np.stack([rng.choice(D, SHARED, replace=False) for _ in range(HEAVY)])
    xb = _rows(rng, N, proto)
    xq = _rows(rng, NQ, proto)                                   # near the prototypes: the long lists are probed
    # centroids: one vector of each prototype (their lists take the prototype's 1200) and vectors of no prototype
    cen = np.ascontiguousarray(np.concatenate([xb[:HEAVY], xb[HEAVY * 1200:HEAVY * 1200 + NLIST - HEAVY]]))
    rank = rng.permutation(N)                                    # rank[id]: the vector's position in key order
    key = (400.0 + 0.25 * rank).astype(np.float32)
    return dict(xb=xb, xq=xq, cen=cen, key=key, built={})


def _built(O, library, fx, ranged):
    """The index of a (storage, kind) and what the oracle searches, built once."""
    from ann_solo_amd import faiss_compat as faiss
    tag = (fx, ranged)
    if tag not in library['built']:
        storage = 'fx22' if fx else 'fp32'
        if ranged:
            idx = faiss.IndexWindowFlat(D, storage=storage)
            idx.add(library['xb'])
            idx.set_window_key(library['key'])
            ref = O.quantize_fx22(library['xb']) if fx else library['xb']
        else:
            idx = faiss.IndexIVFFlat(faiss.IndexFlatIP(D), D, NLIST, storage=storage)
            idx.set_trained(library['cen'])
            idx.add(library['xb'])
            ref = R.host_ivf(O, idx)
            assert (np.diff(ref.list_offsets) > FI_BLK).sum() >= HEAVY
        library['built'][tag] = (idx, ref)
    return library['built'][tag]


@pytest.mark.parametrize('cap,fx,wide,sel,ranged', FORMS)
def test_every_instantiation_equals_the_oracle(O, library, cap, fx, wide, sel, ranged):
    xq = library['xq']
    k, nprobe = (64 if cap == 2048 else 1300), (520 if wide else 8)
    idx, ref = _built(O, library, fx, ranged)
    # which form runs: the postings of the layout the storage asks for, and the dispatcher's shape rules
    assert idx.flat_layout == (2 if fx else 1)
    assert (k + FI_NT + 256 <= 2048) == (cap == 2048) and k + FI_NT + 256 <= cap
    assert (not ranged and nprobe > FI_NT) == wide and nprobe <= NLIST
    what = (cap, fx, wide, sel, ranged)
    if ranged:
        # one window for every query that cuts inside a block at both ends: positions 100 .. 5000 of the key order
        lo, hi = 400.0 + 0.25 * 100, 400.0 + 0.25 * 5000
        assert 0 < 100 % FI_BLK and 0 < 5001 % FI_BLK and 100 // FI_BLK != 5000 // FI_BLK
        W = np.tile(np.array([[lo, hi]], np.float64), (len(xq), 1))
        keep = WR.mask(W[0], library['key'], 0, 0.0, 'interval')
        assert int(keep.sum()) == 4901
        got = idx.search_window(xq, k, W, 0, 0.0, 'interval')
        want = WR.one_list_ivf(O, ref, keep).search(xq, k, 1)
    elif sel:
        keep = np.arange(N) % 3 == 0
        idx.nprobe = nprobe
        idx.set_selector(keep)
        got = idx.search_selected(xq, k)
        idx.set_selector(None)
        want = R.search_selected(O, ref, xq, k, nprobe, keep)
        assert keep[got[1][got[1] >= 0]].all(), what
    else:
        idx.nprobe = nprobe
        got = idx.search(xq, k)
        want = ref.search(xq, k, nprobe)
    R.assert_rows_equal(got, want, what)
    assert (want[1][:, :64] >= 0).all(), what      # (every case has candidates enough to fill 64)
