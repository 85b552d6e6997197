"""numpy restatement of the localisation arithmetic (include/annsolo_mi.h, asl_localize_batch, steps 1-5):
the reference the kernel is compared with bit for bit. Brute force over all peaks for every fragment, no
bisection; ``np.float64`` scalars, every sum sequential."""
import numpy as np

PROTON = np.float64(1.007276466)
H2O = np.float64(18.010565)


def ladders(m, nterm, cterm):
    m = np.asarray(m, np.float64)
    P = np.cumsum(np.concatenate(([np.float64(nterm)], m)))
    S = np.cumsum(np.concatenate(([np.float64(cterm)], m[::-1])))
    return P, S


def fragment_theo(m, nterm, cterm, delta, zmax):
    """theo[type][k][v][z - 1] (k = 0 unused), type 0 = b, 1 = y."""
    P, S = ladders(m, nterm, cterm)
    L = len(m)
    delta = np.float64(delta)
    theo = np.zeros((2, L, 2, zmax), np.float64)
    for k in range(1, L):
        for t in (0, 1):
            plain = P[k] if t == 0 else S[k] + H2O
            for v, base in ((0, plain), (1, plain + delta)):
                for z in range(1, zmax + 1):
                    theo[t, k, v, z - 1] = base / np.float64(z) + PROTON
    return theo


def evidence(mz, intensity, theo, tol, unit):
    """E[type][k][v] (float64) and C[type][k][v] (int) of step 3, plus the peak that served every
    (type, k, v, z) (``pick``, -1: none) for the tests that ask which peak won."""
    x = np.asarray(mz, np.float32).astype(np.float64)
    it = np.asarray(intensity, np.float32)
    tol = np.float64(tol)
    t = theo.reshape(-1)
    R = np.full(len(t), tol) if unit == 'Da' else (tol * np.float64(1e-6)) * t
    pick = np.full(len(t), -1, np.int64)
    chunk = max(1, (1 << 21) // max(len(x), 1))
    for a in range(0, len(t) if len(x) else 0, chunk):      # every peak against every fragment
        with np.errstate(invalid='ignore'):
            d = x[None, :] - t[a:a + chunk, None]
            hit = (-R[a:a + chunk, None] <= d) & (d <= R[a:a + chunk, None])
        best = np.argmax(np.where(hit, it[None, :], -np.inf), axis=1)    # the first of the largest
        pick[a:a + chunk] = np.where(hit.any(axis=1), best, -1)
    pick = pick.reshape(theo.shape)
    pick[:, 0] = -1                                # (k = 0 is no fragment)
    contrib = np.where(pick >= 0, it[np.maximum(pick, 0)].astype(np.float64) if len(it) else 0.0, 0.0)
    E = np.zeros(theo.shape[:3], np.float64)
    for z in range(theo.shape[3]):                 # in charge order, from 0.0
        E = E + contrib[..., z]
    return E, (pick >= 0).sum(axis=3), pick


def localize_ref(mz, intensity, residue_mass, nterm, cterm, zmax, delta, tol, unit):
    """One SSM: a dict with site_score (float64 [L]), site_count (int32 [L]) and the summary."""
    m = np.asarray(residue_mass, np.float64)
    L = len(m)
    theo = fragment_theo(m, nterm, cterm, delta, int(zmax))
    E, C, pick = evidence(mz, intensity, theo, tol, unit)

    def total(vb, vy):      # vb(k), vy(k): the variant of b_k / y_k
        s, c = np.float64(0.0), 0
        for k in range(1, L):
            s = s + E[0, k, vb(k)]
            s = s + E[1, k, vy(k)]
            c += int(C[0, k, vb(k)]) + int(C[1, k, vy(k)])
        return s, c
    score, count = np.zeros(L, np.float64), np.zeros(L, np.int32)
    for j in range(L):
        score[j], count[j] = total(lambda k: int(k >= j + 1), lambda k: int(k >= L - j))
    none_score, none_count = total(lambda k: 0, lambda k: 0)
    best = score.max()
    tied = np.nonzero(score == best)[0]
    below = score[score < best]
    return dict(site_score=score, site_count=count, best_lo=int(tied[0]), best_hi=int(tied[-1]),
                n_best=len(tied), best_count=int(count[tied[0]]), best_score=best,
                runner_score=below.max() if len(below) else best, none_score=none_score,
                none_count=none_count, pick=pick, theo=theo)
