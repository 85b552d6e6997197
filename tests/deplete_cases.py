"""Case generators of the depletion / chimeric-search tests (tests/test_deplete_cpu.py on the reference and
the oracle-backed engine, tests/test_gpu_deplete.py on the device): single SSMs, mixed batches over the size
grid, and the small planted world both engine tests run."""
import numpy as np

import deplete_ref as R

Q_PEAKS = (0, 1, 2, 63, 64, 65, 128, 256, 257, 1024, 4096)
L_PEAKS = (1, 50, 64, 65, 256, 4096)
# the rescoring states no largest charge (rescore.hpp); its kernels change path above 4 (the flat kernel's shift
# table) and at 31 (to the binary-search kernel), and the oracle's shift table ends at 63
CHARGES = (1, 2, 3, 5, 31, 63)
FLAGS = (0, R.SCORE_SHIFT, R.SCORE_FRAGMENT_PPM, R.SCORE_SHIFT | R.SCORE_FRAGMENT_PPM)
PMD_KINDS = ('zero', 'gate-', 'gate+', 15.994915, -150.0, 500.0)


def tol_of(flags):
    return 20.0 if flags & R.SCORE_FRAGMENT_PPM else 0.02


def reach(mz, tol, flags):
    return tol * 1e-6 * mz if flags & R.SCORE_FRAGMENT_PPM else tol


def gate_precursors(l_pmz, z, tol, flags):
    """(closed, open): two neighbouring doubles for the query's precursor m/z, the largest for which the shift
    gate of the contract is closed and the next one, for which it is open."""
    is_open = lambda v: R.shifts_of(v, l_pmz, z, tol, flags | R.SCORE_SHIFT)[0] > 1
    lo, hi = np.float64(l_pmz), np.float64(l_pmz) + 1.0        # |pmd| - gate ascends with q above l_pmz: bisect
    assert not is_open(lo) and is_open(hi)
    while np.nextafter(lo, np.inf) < hi:
        mid = lo + (hi - lo) / 2.0
        lo, hi = (lo, mid) if is_open(mid) else (mid, hi)
    return float(lo), float(hi)


def query_precursor(kind, l_pmz, z, tol, flags):
    if kind == 'zero':
        return float(l_pmz)
    if kind in ('gate-', 'gate+'):
        return gate_precursors(l_pmz, z, tol, flags)[kind == 'gate+']
    return float(l_pmz) + float(kind) / z


def make_ssm(rng, qn, ln, z, kind, flags, annotate='mixed'):
    """One SSM as a dict: a library row of ``ln`` peaks and a query of ``qn`` peaks drawn around it -- peaks
    near a library peak, near one of its shifted positions (either side of the window's edge), and noise."""
    tol = tol_of(flags)
    l_mz = np.sort(rng.uniform(200.0, 1500.0, ln)).astype(np.float32)
    if annotate == 'none':
        l_chg = np.zeros(ln, np.uint8)
    else:
        l_chg = rng.integers(0, min(z, 3) + 1, ln).astype(np.uint8)
    l_pmz = float(rng.uniform(400.0, 900.0))
    q_pmz = query_precursor(kind, l_pmz, z, tol, flags)
    pmd = (q_pmz - l_pmz) * z
    how = rng.integers(0, 3, qn)
    j = rng.integers(0, ln, qn)
    c = rng.integers(1, z + 1, qn)
    base = l_mz[j].astype(np.float64)
    x = np.where(how == 0, base, np.where(how == 1, base + pmd / c, rng.uniform(200.0, 1500.0, qn)))
    x = x + rng.uniform(-1.5, 1.5, qn) * reach(np.abs(x), tol, flags) * (how < 2)
    q_mz = np.sort(x.astype(np.float32))
    q_int = rng.uniform(0.01, 1.0, qn).astype(np.float32)
    return dict(q_mz=q_mz, q_int=q_int, q_pmz=q_pmz, l_mz=l_mz, l_int=rng.uniform(0.01, 1.0, ln).astype(np.float32),
                l_chg=l_chg, l_pmz=l_pmz, z=int(z))


def pack(ssms, lib_charge=True, skip=()):
    """(queries, library, lib_rows): packed numpy tuples, one library row per SSM (shuffled: row != s), rows of
    the SSMs in ``skip`` set to -1."""
    n = len(ssms)
    perm = np.random.default_rng(n).permutation(n)            # SSM s -> library row perm[s]
    inv = np.argsort(perm)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    qo = np.concatenate([[0], np.cumsum([len(s['q_mz']) for s in ssms])]).astype(np.int32)
    queries = (qo, cat([s['q_mz'] for s in ssms], np.float32), cat([s['q_int'] for s in ssms], np.float32),
               np.zeros(int(qo[-1]), np.uint8), np.array([s['q_pmz'] for s in ssms], np.float64),
               np.array([s['z'] for s in ssms], np.int32))
    lib = [ssms[i] for i in inv]
    lo = np.concatenate([[0], np.cumsum([len(s['l_mz']) for s in lib])]).astype(np.int32)
    library = (lo, cat([s['l_mz'] for s in lib], np.float32), cat([s['l_int'] for s in lib], np.float32),
               cat([s['l_chg'] for s in lib], np.uint8) if lib_charge else None,
               np.array([s['l_pmz'] for s in lib], np.float64), np.array([s['z'] for s in lib], np.int32))
    rows = perm.astype(np.int64)
    rows[list(skip)] = -1
    return queries, library, rows


def grid_batch(fi, annotate='mixed'):
    """About 100 SSMs for flag word FLAGS[fi]: every (query peaks, library peaks) pair of the grid once, charges
    and precursor differences cycling through theirs (large pairs keep to small charges: the reference tests
    every triple), then every charge against every precursor difference at 65 x 50 peaks. One call so mixes
    wave packing, staged and unstaged rows."""
    flags = FLAGS[fi]
    rng = np.random.default_rng(1000 + fi)
    out, t = [], fi
    for qn in Q_PEAKS:
        for ln in L_PEAKS:
            z = CHARGES[t % len(CHARGES)]
            if qn * ln > (1 << 18):
                z = CHARGES[t % 3]
            out.append(make_ssm(rng, qn, ln, z, PMD_KINDS[(t // 2) % len(PMD_KINDS)], flags, annotate))
            t += 1
    for z in CHARGES:
        for kind in PMD_KINDS:
            out.append(make_ssm(rng, 65, 50, z, kind, flags, annotate))
    return out


# ------------------------------------------------------------------------------------ the planted world
TOL = 0.02
N_LIB, N_QUERIES, N_PLANTED, N_SAME = 300, 64, 32, 4
PEAKS = 30
FAR = 63           # the query whose partner lies outside chimeric_window, inside its isolation window


def world(isolation=False):
    """(library pack, {2: query pack}, query_meta, library_meta, config kwargs, plan): 300 library spectra of
    charge 2 and 64 queries. Row s has 30 peaks at 200 + 40 k + 0.1 s (k = 0..29): peaks of different rows are
    0.1 = 5 tolerances apart or more, and so are they from the positions row s - 1 reaches when it is shifted
    by 0.3 or 0.6. Its precursor m/z is 500 + 0.5 s, its peptide its own -- except rows 201, 209, 217, 225, which
    share the peptide of the row below them.
      queries 0..31:  A = row 10 + 6 i and 0.6 x B = row A + 1 (0.5 m/z above A); the odd ones sit 0.3 m/z above
                      A's precursor (found by the open level, pmd = 0.6: shifts 0.6 and 0.3), the even ones on it
      queries 32..35: A = 200 + 8 i and 0.6 x row A + 1 of the SAME peptide: the residue level drops the match
      queries 36..62: A alone (three of four with 3 noise peaks: residues that are no valid spectrum)
      query 63:       A = row 280 and 0.6 x row 284, 2.0 m/z above: outside chimeric_window = 2.0, inside the
                      isolation window of +-3 that ``isolation=True`` gives every query
    ``plan``: per query (A, B or -1)."""
    from ann_solo_amd.packed import PackedSpectra
    rng = np.random.default_rng(77)
    k = np.arange(PEAKS)
    l_mz = (200.0 + 40.0 * k[None, :] + 0.1 * np.arange(N_LIB)[:, None]).astype(np.float32)
    rank = np.stack([rng.permutation(PEAKS) + 1 for _ in range(N_LIB)]).astype(np.float32)
    l_int = (rank / np.sqrt((rank.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(np.float32)
    l_chg = ((k[None, :] + np.arange(N_LIB)[:, None]) % 3).astype(np.uint8)
    l_pmz = 500.0 + 0.5 * np.arange(N_LIB)
    lib = PackedSpectra.from_numpy(np.arange(N_LIB + 1) * PEAKS, l_mz.ravel(), l_int.ravel(), l_chg.ravel(),
                                   l_pmz, np.full(N_LIB, 2))
    peptide = [f'PEP{r}K' for r in range(N_LIB)]
    plan = []
    for i in range(N_QUERIES):
        if i < N_PLANTED:
            plan.append((10 + 6 * i, 11 + 6 * i))
        elif i < N_PLANTED + N_SAME:
            a = 200 + 8 * (i - N_PLANTED)
            peptide[a + 1] = peptide[a]
            plan.append((a, a + 1))
        elif i == FAR:
            plan.append((280, 284))
        else:
            plan.append((3 + 7 * (i - 36), -1))
    q_mz, q_int, q_pmz, offs = [], [], [], [0]
    for i, (a, b) in enumerate(plan):
        mz, it = [l_mz[a]], [l_int[a]]
        if b >= 0:
            mz.append(l_mz[b])
            it.append(np.float32(0.6) * l_int[b])
        elif i % 4:
            mz.append(np.array([333.33, 777.77, 1111.11], np.float32) + np.float32(0.013 * i))
            it.append(np.full(3, 0.05, np.float32))
        mz, it = np.concatenate(mz), np.concatenate(it)
        order = np.argsort(mz, kind='stable')
        it = it[order]
        q_mz.append(mz[order])
        q_int.append((it / np.sqrt((it.astype(np.float64) ** 2).sum())).astype(np.float32))
        q_pmz.append(l_pmz[a] + (0.3 if i % 2 else 0.0))
        offs.append(offs[-1] + len(mz))
    q = PackedSpectra.from_numpy(np.array(offs), np.concatenate(q_mz), np.concatenate(q_int), None,
                                 np.array(q_pmz), np.full(N_QUERIES, 2))
    qmeta = {2: [dict(identifier=f'scan={i}', index=i, precursor_charge=2, precursor_mz=float(q_pmz[i]))
                 for i in range(N_QUERIES)]}
    if isolation:
        for i, m in enumerate(qmeta[2]):
            m['isolation_window'] = (q_pmz[i] - 3.0, q_pmz[i] + 3.0)
    pmz32 = l_pmz.astype(np.float32)
    lmeta = {2: [dict(identifier=int(r), peptide=peptide[r], precursor_mz=float(pmz32[r])) for r in range(N_LIB)]}
    kw = dict(mode='bf', batch_size=16, precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm',
              precursor_tolerance_mass_open=300.0, precursor_tolerance_mode_open='Da', fragment_mz_tolerance=TOL,
              chimeric_window=2.0)
    return lib, {2: q}, qmeta, lmeta, kw, plan


def reference_level(O, base, lib, queries, qmeta, lmeta, cfg, cosines=None):
    """The residue level of the contract on top of the table ``base`` (the engine's with the switch off), by the
    reference depletion and the oracle's dot product alone: rows (qrow, lib_row, score, explained_intensity) in
    the order the engine files them. ``cosines``: the search-engine score over the residues and the oracle's peak
    matches, called as ``spectrum_similarity.ssm_cosine`` is (default: ``oracle_backend.oracle_cosines``; the
    device test passes the device's, whose fp64 sum is a tree)."""
    from ann_solo_amd.packed import PackedSpectra
    from ann_solo_amd.spectral_library import isolation_windows
    from ann_solo_amd.spectrum_match import score_flags
    if cosines is None:
        from oracle_backend import oracle_cosines as cosines
    L, Q = O.Spectra(*lib.numpy()), O.Spectra(*queries[2].numpy())
    pmz32 = L.precursor_mz.astype(np.float32).astype(np.float64)
    flags = score_flags(cfg.allow_peak_shifts, cfg.fragment_tolerance_unit)
    iso = isolation_windows(qmeta[2], Q.n)
    rows, res_mz, res_int, offs, pairs = [], [], [], [0], []
    for i in np.nonzero(base.q < cfg.fdr)[0]:
        qr, lr = int(base.qrow[i]), int(base.lib_row[i])
        qmz, qit, _ = Q.peaks(qr)
        lmz, _, lch = L.peaks(lr)
        one = R.deplete_one(qmz, qit, Q.precursor_mz[qr], lmz, lch, L.precursor_mz[lr], 2, cfg.fragment_mz_tolerance,
                            flags, cfg.min_peaks, cfg.min_mz_range)
        if not one['valid']:
            continue
        lo, hi = iso[qr] if iso is not None else (Q.precursor_mz[qr] - cfg.chimeric_window / 2.0,
                                                   Q.precursor_mz[qr] + cfg.chimeric_window / 2.0)
        cand = np.nonzero((lo <= pmz32) & (pmz32 <= hi))[0].astype(np.int64)
        if len(cand) == 0:
            continue
        res = O.Spectra([0, one['count']], one['mz'], one['intensity'], None, [Q.precursor_mz[qr]], [2])
        b, _, m = O.best_match(res, 0, L, cand, cfg.fragment_mz_tolerance, False)
        if b < 0:
            continue
        row = int(cand[b])
        if lmeta[2][row]['peptide'] == lmeta[2][lr]['peptide']:
            continue
        rows.append((qr, row, 1.0 - float(np.float64(one['energy']))))
        res_mz.append(one['mz'])
        res_int.append(one['intensity'])
        offs.append(offs[-1] + one['count'])
        pairs.append(m)
    if not rows:
        return []
    n = len(rows)
    pack = PackedSpectra.from_numpy(np.array(offs), np.concatenate(res_mz), np.concatenate(res_int), None,
                                    np.array([Q.precursor_mz[r[0]] for r in rows]), np.full(n, 2))
    stride = max(1, max(len(m) for m in pairs))
    pm = np.zeros((n, stride, 2), np.uint32)
    for k, m in enumerate(pairs):
        pm[k, :len(m)] = m
    cnt = np.array([len(m) for m in pairs], np.int32)
    score = np.asarray(cosines(pack, lib, np.array([r[1] for r in rows], np.int32), pm, cnt), np.float64)
    return [(qr, row, float(score[k]), ex) for k, (qr, row, ex) in enumerate(rows)]
