"""numpy restatement of the decoy arithmetic (include/annsolo_mi.h, asl_decoy_batch, steps 1-5): the
reference the kernel is compared with bit for bit. Ladders by ``np.cumsum`` (sequential), every fragment
of every series scanned for every peak, no search structure."""
import numpy as np

PROTON = 1.007276466
CO = 27.994915
H2O = 18.010565
LOSSES = np.array([0.0, -1.007825, -17.026549, -18.010565, -27.994915, -43.989829, -45.021464,
                   -46.005479, -63.998301, -79.956818, -79.966331, -91.009195, -91.993211, -97.976896])
TYPE_NAMES = ('', 'a', 'b', 'p', 'y')


def ladders(m, nterm, cterm):
    m = np.asarray(m, np.float64)
    P = np.cumsum(np.concatenate(([np.float64(nterm)], m)))
    S = np.cumsum(np.concatenate(([np.float64(cterm)], m[::-1])))
    return P, S


def fragment_table(m, nterm, cterm, zmax):
    """Every theoretical fragment in tie-break order (type, n, z, loss): columns type, n, z, loss and
    the base mass; ``theo`` from ``theo_of``."""
    P, S = ladders(m, nterm, cterm)
    L = len(m)
    rows = []
    for t in (1, 2, 3, 4):
        for n in ([L] if t == 3 else range(1, L)):
            if t == 1:
                base = P[n] - CO
            elif t == 2:
                base = P[n]
            elif t == 3:
                base = (P[L] + np.float64(cterm)) + H2O
            else:
                base = S[n] + H2O
            for z in range(1, zmax + 1):
                for l in range(len(LOSSES)):
                    rows.append((t, n, z, l, base))
    a = np.asarray(rows, np.float64).reshape(-1, 5)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2].astype(np.int64), \
        a[:, 3].astype(np.int64), a[:, 4]


def theo_of(base, loss_idx, z):
    return (base + LOSSES[loss_idx]) / z.astype(np.float64) + PROTON


def decoy_ref(mz, intensity, residue_mass, perm, nterm, cterm, zmax, tol, unit, chunk=128):
    """One spectrum. Returns a dict: mz (float32), intensity, src, charge (decoy order) and ann_type /
    ann_n / ann_z / ann_loss (raw order)."""
    mz = np.asarray(mz, np.float32)
    intensity = np.asarray(intensity, np.float32)
    m = np.asarray(residue_mass, np.float64)
    perm = np.asarray(perm, np.int64)
    n = len(mz)
    ft, fn, fz, fl, fbase = fragment_table(m, nterm, cterm, int(zmax))
    theo = theo_of(fbase, fl, fz)
    _, _, _, _, dbase = fragment_table(m[perm], nterm, cterm, int(zmax))
    theo_d = theo_of(dbase, fl, fz)
    x = mz.astype(np.float64)
    pick = np.full(n, -1, np.int64)
    reach = np.full(len(theo), float(tol)) if unit == 'Da' else (float(tol) * 1e-6) * theo
    for a in range(0, n, chunk):
        xx = x[a:a + chunk, None]
        with np.errstate(invalid='ignore'):
            hit = np.abs(xx - theo[None, :]) <= reach[None, :]
        cand = np.where(hit, theo[None, :], np.inf)
        j = np.argmin(cand, axis=1)               # first of the lowest: the enumeration is the tie order
        ok = hit[np.arange(len(j)), j]
        pick[a:a + chunk] = np.where(ok, j, -1)
    ann = pick >= 0
    p = np.where(ann, pick, 0)
    new = np.where(ann, theo_d[p] + (x - theo[p]), x)
    order = np.lexsort((np.arange(n), new))
    z = np.where(ann, fz[p], 0)
    return dict(mz=new[order].astype(np.float32), intensity=intensity[order], src=order.astype(np.int32),
                charge=z[order].astype(np.uint8),
                ann_type=np.where(ann, ft[p], 0).astype(np.uint8), ann_n=np.where(ann, fn[p], 0).astype(np.uint8),
                ann_z=z.astype(np.uint8), ann_loss=np.where(ann, fl[p], 0).astype(np.uint8),
                new_f64=new[order])
