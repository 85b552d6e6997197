"""Named score regimes for the scans' fused top-k (a helper, not a test).

The list scans select their k best hits through a 512-bucket score histogram over the documented range
[-0.25, 1) (``csrc/hist_topk.hpp``); scores outside it clamp to the end buckets and a crowded threshold
bucket falls back to exact sort-and-truncate flushes. Every regime here is ONE seeded world -- sparse rows
of 40 random non-zeros plus 4 hot dimensions that every row shares, so no inner product is near 0 --
scaled by a power of two or with signs changed, so that the scores leave that range, crowd one bucket or
straddle its edges while the oracle's arithmetic stays exactly the control's (a power-of-two scaling moves
exponents only). tests/test_score_range_cases_cpu.py holds every regime to its property with the oracle and
float64 brute force; tests/test_gpu_score_range.py holds the kernels to the oracle on them."""
import numpy as np

D = 800
N = 6000
NQ = 16
NLIST = 4
NNZ = 40                 # random non-zeros of a row ...
HOT = 4                  # ... plus the dimensions every row shares: 44 <= 64 non-zeros, every sparse form applies
PQ_M = 32
PQ_KSUB = 256
PQ_NITER = 2
PQ_SEED = 4242
WIDE_NLIST = 600
SEED = 20266

# the k of every comparison: both key-buffer sizes (k <= 1280 and beyond), their boundary, the largest
# single-pass k and one bounded-pass k
KS = (1, 100, 1024, 1280, 1281, 2048, 2500)

HIST_LO, HIST_HI = -0.25, 1.0          # the documented bucket range
BUCKET_WIDTH = 1.25 / 512

# regime -> (power-of-two scale of the library side: vectors, centroids, codebooks; scale of the queries).
# The centroids and codebooks take the vectors' scale, so lists, probes and PQ codes are the control's and
# every score is the control's times a power of two (tests/test_score_range_cases_cpu.py checks the bits).
#   unit        control: scores in about [0.28, 0.6]
#   across_one  scores in about [0.57, 1.2]: clamped and unclamped candidates in one row
#   above_one   every score >= 1: all in the top bucket
#   negated     every score < -0.24: the bottom bucket(s)
#   far_below   every score < -0.25: the bottom bucket, the threshold bucket stays 0
#   tiny        scores about 1e-13 (normal numbers): all in one interior bucket
#   signed      a random half of the library rows negated: scores on both sides of 0 and of -0.25
#   one_bucket  N copies of one row, each non-zero times 1 + 2e-4 N(0, 1): thousands of distinct scores
#               within two adjacent buckets
#   wide_lists  the control under 600 lists and 600 probes: the two-probes-per-thread forms
_SCALE = {
    'unit': (1.0, 1.0),
    'across_one': (2.0, 1.0),
    'above_one': (8.0, 8.0),
    'negated': (1.0, -1.0),
    'far_below': (8.0, -8.0),
    'tiny': (2.0 ** -40, 1.0),
    'signed': (1.0, 1.0),
    'one_bucket': (1.0, 1.0),
    'wide_lists': (1.0, 1.0),
}
REGIMES = tuple(_SCALE)
# the codebooks of `one_bucket` are the control's scaled down to the size of its residuals (the planted
# 2e-4 relative noise): with the control's own every near-copy would take the same code and the ADC
# scores would be the already-covered bit-identical case
ONE_BUCKET_CB_SCALE = 2.0 ** -9
# regimes whose stored components lie in [0, 1): the fixed-point storage keeps 4-byte postings on them
FX22_REGIMES = ('unit', 'across_one', 'negated', 'tiny', 'one_bucket')


def _rows(rng, m, hot_dims):
    x = np.zeros((m, D), np.float32)
    rest = np.setdiff1d(np.arange(D), hot_dims)
    for i in range(m):
        cols = rng.choice(rest, size=NNZ, replace=False)
        x[i, cols] = (rng.random(NNZ) + 0.05).astype(np.float32)
    x[:, hot_dims] = (rng.random((m, HOT)) + 1.2).astype(np.float32)
    x /= np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(x, np.float32)


_WORLD = {}


def world(seed=SEED):
    """(xb [N, D], xq [NQ, D]) of the control, L2-normalised, non-negative."""
    if seed not in _WORLD:
        rng = np.random.default_rng(seed)
        hot_dims = np.sort(rng.choice(D, size=HOT, replace=False))
        _WORLD[seed] = (_rows(rng, N, hot_dims), _rows(rng, NQ, hot_dims))
    return _WORLD[seed]


def regime(name, seed=SEED):
    """(xb, xq, centroids, nlist) of one regime; the arrays are fresh copies."""
    xb, xq = world(seed)
    sb, sq = _SCALE[name]
    rng = np.random.default_rng(seed + 1)
    if name == 'signed':
        xb = xb.copy()
        xb[rng.permutation(N)[:N // 2]] *= np.float32(-1.0)
    elif name == 'one_bucket':
        noise = 1.0 + 2e-4 * rng.standard_normal((N, D))
        xb = (xb[:1].astype(np.float64) * noise).astype(np.float32)
    nlist = WIDE_NLIST if name == 'wide_lists' else NLIST
    cen = xb[:nlist]
    f = np.float32
    return (np.ascontiguousarray(xb * f(sb)), np.ascontiguousarray(xq * f(sq)),
            np.ascontiguousarray(cen * f(sb)), nlist)


def build_regimes(seed=SEED):
    """[(name, xb, xq, centroids)] in the order of REGIMES."""
    return [(name,) + regime(name, seed)[:3] for name in REGIMES]


_CB = {}


def unit_codebooks(O, seed=SEED):
    """(by-residual codebooks, raw-vector codebooks) [PQ_M, PQ_KSUB, D / PQ_M] trained once, by the oracle,
    on the control."""
    if seed not in _CB:
        xb, _, cen, _ = regime('unit', seed)
        cb = O.pq_train(xb, cen, PQ_M, PQ_KSUB, PQ_NITER, PQ_SEED)
        raw = O.pq_train(xb, np.zeros((1, D), np.float32), PQ_M, PQ_KSUB, PQ_NITER, PQ_SEED)
        _CB[seed] = (cb, raw)
    return _CB[seed]


def codebooks(O, name, seed=SEED):
    """The control's codebooks under the regime's own power-of-two scaling: (by-residual, raw)."""
    cb, raw = unit_codebooks(O, seed)
    s = np.float32(_SCALE[name][0])
    if name == 'one_bucket':
        return cb * np.float32(ONE_BUCKET_CB_SCALE), raw.copy()
    return cb * s, raw * s


def host_indexes(O, name, seed=SEED):
    """The oracle's side of a regime: dict(xb, xq, cen, nlist, cb, raw_cb, assign, flat, pq, raw) with
    ``flat`` / ``pq`` / ``raw`` the ``O.HostIVF`` over the vectors, the by-residual codes and the raw codes."""
    import raw_pq_ref as R
    xb, xq, cen, nlist = regime(name, seed)
    cb, raw_cb = codebooks(O, name, seed)
    a = O.assign(xb, cen, 0)
    return dict(name=name, xb=xb, xq=xq, cen=cen, nlist=nlist, cb=cb, raw_cb=raw_cb, assign=a,
                flat=O.HostIVF(cen, a, xb),
                pq=O.HostIVF(cen, a, O.pq_encode(xb, cen, a, cb), cb),
                raw=O.HostIVF(cen, a, R.raw_codes(O, xb, raw_cb), raw_cb))
