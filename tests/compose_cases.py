"""The composition tests' shared side (tests/test_compose_cases_cpu.py on the host, tests/test_gpu_compose.py on
the device): one small planted world, written as ``.sptxt`` / ``.mgf`` text and read back by the host readers
(tests/sptxt_ref.py, tests/mgf_ref.py) -- so the objects and the files hold the same numbers by construction --,
the bases (configurations that change results: a pairwise covering array over four axes), the overlays
(switches documented NOT to change results) and, as data, what every overlay owns and must leave alone."""
import itertools

import numpy as np

import decoy_cases as DC
import decoy_ref
import localize_cases as LC
import mgf_ref
import sptxt_ref

# ------------------------------------------------------------------------------------------------ the world
SEED = 2024
# charge 2 / charge 3 spectra; of the charge-2 ones N_PAIRS are isobaric twins of the first rows and N_REPEAT a second
# spectrum of the peptide of the rows behind those (the first plain queries: distinct_matches has work)
N_LIB2, N_LIB3, N_PAIRS, N_REPEAT = 300, 140, 24, 16    # (charge 3 with its decoys: 2^pq_bits vectors to train on)
N_PLAIN2, N_PLAIN3, N_MOD, N_FOREIGN, N_UNKNOWN = 90, 40, 140, 120, 12
DELTAS = (15.994915, 42.010565, 79.966331, -17.026549)
ISOLATION = (-45.0, 12.0)                    # (lo, hi) around the query's precursor m/z: holds every delta at z = 2
MAX_PEAKS_USED = 80                          # (the one query of 75 peaks keeps more than 64 hash components)

# what every engine of the tests is built with (tests/test_gpu_device_fdr.py's sizes)
ENGINE = dict(num_list=8, num_probe=8, num_candidates=64, kmeans_niter=4, fragment_mz_tolerance=0.02,
              decoy_tolerance_unit='Da', seed=5, min_mz_range=100.0, fdr=0.05, fdr_min_group_size=20,
              precursor_tolerance_mass=20.0, precursor_tolerance_mode='ppm', max_peaks_used=MAX_PEAKS_USED,
              chimeric_window=2.0)


def _peptide(rng, length):
    return DC.random_peptide(rng, length, mod_p=0.0)


def _spectrum(rng, pep, z, n_noise=12):
    """A complete singly charged b / y ladder of ``pep`` and ``n_noise`` weak noise peaks."""
    masses = LC.parse(pep).masses
    b, y = LC.ladder_mz(masses, 0, 0.0)
    frag = np.concatenate((b, y))
    ann = [f'b{k + 1}/0.00' for k in range(len(b))] + [f'y{k + 1}/0.00' for k in range(len(y))]
    noise = rng.uniform(120.0, max(400.0, float(masses.sum())), n_noise)
    mz = np.concatenate((frag, noise))
    inten = np.concatenate((rng.lognormal(5.0, 0.8, len(frag)), rng.lognormal(3.0, 0.4, n_noise)))
    pmz = (float(masses.sum()) + decoy_ref.H2O + z * decoy_ref.PROTON) / z
    return dict(peptide=pep, masses=masses, z=z, pmz=pmz, mz=mz, intensity=inten, ann=ann + ['?'] * n_noise,
                n_frag=len(frag))


def _record(i, s):
    """One record in the shape SpectraST writes (as tests/sptxt_cases.py's ``record``), Mods=0."""
    order = np.argsort(s['mz'], kind='stable')
    lines = ['Name: %s/%d' % (s['peptide'], s['z']), 'LibID: %d' % i, 'MW: %.4f' % (s['pmz'] * s['z']),
             'PrecursorMZ: %.4f' % s['pmz'], 'Status: Normal', 'FullName: K.%s.L/%d (CID)' % (s['peptide'], s['z']),
             'Comment: AvePrecursorMz=%.4f Fullname=K.%s.L/%d Mods=0 Protein=1/sp|P%05d|TARGET_X Spec=Consensus'
             % (s['pmz'] + 0.3, s['peptide'], s['z'], i), 'NumPeaks: %d' % len(order)]
    lines += ['%.4f\t%.1f\t%s\t5/9 0.3' % (s['mz'][k], s['intensity'][k], s['ann'][k]) for k in order]
    return '\n'.join(lines + ['']) + '\n'


def _block(title, pmz, z, mz, inten, rt):
    order = np.argsort(mz, kind='stable')
    lines = ['BEGIN IONS', f'TITLE={title}', 'PEPMASS=%.5f' % pmz, 'RTINSECONDS=%.1f' % rt]
    if z is not None:
        lines.append(f'CHARGE={z}+')
    lines += ['%.4f %.2f' % (mz[k], inten[k]) for k in order]
    return '\n'.join(lines + ['END IONS']) + '\n'


def _noisy(rng, s, keep_p=0.9, sigma=0.003, scale=1.0):
    keep = rng.random(len(s['mz'])) < keep_p
    n = int(keep.sum())
    return s['mz'][keep] + rng.normal(0.0, sigma, n), scale * s['intensity'][keep] * rng.uniform(0.8, 1.25, n)


_WORLD = {}


def world(seed=SEED):
    """dict(sptxt, mgf: the two files as bytes; library, queries: what the host readers make of them; kind[i]:
    the kind of query i -- 'plain', 'mod', 'mix', 'foreign', 'unknown', 'empty', 'wide' --; planted[i]: per query
    the library record numbers (1-based, the identifiers of the sptxt reader) it was built from, and for 'mod'
    (record, site, delta)). Built once per seed."""
    if seed in _WORLD:
        return _WORLD[seed]
    rng = np.random.default_rng(seed)
    lib = []
    n_unique = N_LIB2 - N_PAIRS - N_REPEAT
    assert N_PAIRS + N_PLAIN2 + N_MOD <= n_unique
    for i in range(n_unique):
        lib.append(_spectrum(rng, _peptide(rng, int(rng.integers(9, 20))), 2))
    for i in range(N_PAIRS):            # an isobaric twin: the same residues in another order, the same precursor
        a = lib[i]
        seq = list(a['peptide'])
        while True:
            perm = rng.permutation(len(seq) - 1)
            twin = ''.join(seq[k] for k in perm) + seq[-1]
            if twin != a['peptide']:
                break
        lib.append(_spectrum(rng, twin, 2))
    for i in range(N_REPEAT):           # another spectrum of a peptide the library holds already
        lib.append(_spectrum(rng, lib[N_PAIRS + i]['peptide'], 2))
    for i in range(N_LIB3):
        lib.append(_spectrum(rng, _peptide(rng, int(rng.integers(14, 24))), 3))
    sptxt = ''.join(_record(i + 1, s) for i, s in enumerate(lib)).encode()
    twins = [(i, n_unique + i) for i in range(N_PAIRS)]
    c3 = list(range(N_LIB2, N_LIB2 + N_LIB3))
    blocks, kind, planted = [], [], []

    def add(k, plan, pmz, z, mz, inten):
        j = len(blocks)
        blocks.append(_block(f'scan={j}', pmz, z, np.asarray(mz), np.asarray(inten), 0.5 * j))
        kind.append(k)
        planted.append(plan)
    for i in range(N_PLAIN2):                       # noisy unmodified copies (the first N_REPEAT: of a peptide with two spectra)
        s = lib[N_PAIRS + i]
        add('plain', (N_PAIRS + i + 1,), s['pmz'], 2, *_noisy(rng, s))
    for i in range(N_PLAIN3):
        s = lib[c3[i]]
        add('plain', (c3[i] + 1,), s['pmz'], 3, *_noisy(rng, s))
    for i in range(N_MOD):                          # a modification mass on a known residue
        r = N_PAIRS + N_PLAIN2 + i
        s = lib[r]
        delta, site = DELTAS[i % len(DELTAS)], int(rng.integers(1, len(s['masses']) - 1))
        b, y = LC.ladder_mz(s['masses'], site, delta)
        frag = np.concatenate((b, y)) + rng.normal(0.0, 0.003, s['n_frag'])
        mz = np.concatenate((frag, s['mz'][s['n_frag']:]))
        add('mod', (r + 1, site, delta), s['pmz'] + delta / 2.0, 2, mz, s['intensity'] * rng.uniform(0.8, 1.25, len(mz)))
    for a, b in twins:                              # two library peptides in one isolation window
        ma, ia = _noisy(rng, lib[a], keep_p=1.0)
        mb, ib = _noisy(rng, lib[b], keep_p=1.0, scale=0.6)
        add('mix', (a + 1, b + 1), lib[a]['pmz'], 2, np.concatenate((ma, mb)), np.concatenate((ia, ib)))
    for i in range(N_FOREIGN):                      # peptides the library does not hold, at precursors it does
        host = lib[int(rng.integers(N_LIB2))]
        s = _spectrum(rng, _peptide(rng, int(rng.integers(9, 20))), 2)
        add('foreign', (), host['pmz'] * (1.0 + 2e-6 * rng.normal()), 2, s['mz'], s['intensity'])
    for i in range(N_UNKNOWN):                      # no CHARGE line: tried at 2 and at 3
        r = c3[N_PLAIN3 + i // 2] if i % 2 else N_PAIRS + i
        add('unknown', (r + 1,), lib[r]['pmz'], None, *_noisy(rng, lib[r]))
    add('empty', (), 500.0, 2, np.zeros(0), np.zeros(0))
    add('wide', (), lib[N_PAIRS]['pmz'] + 3.0, 2, 150.0 + 17.31 * np.arange(75), rng.uniform(50.0, 100.0, 75))
    mgf = ''.join(blocks).encode()
    out = dict(sptxt=sptxt, mgf=mgf, library=sptxt_ref.read_sptxt(sptxt), queries=mgf_ref.read_mgf(mgf),
               kind=np.array(kind), planted=planted)
    assert len(out['library']) == len(lib) and len(out['queries']) == len(blocks)
    _WORLD[seed] = out
    return out


def add_isolation_windows(query_meta):
    """``isolation_window`` on every query record (in place): ISOLATION around its precursor m/z."""
    for metas in query_meta.values():
        for m in metas:
            m['isolation_window'] = (m['precursor_mz'] + ISOLATION[0], m['precursor_mz'] + ISOLATION[1])
    return query_meta


# ------------------------------------------------------------------------------------------------ the bases
# name -> Config keywords; 'isolation' is no Config field: the queries' metadata carry the windows
AXES = {
    'index': {
        'ivfflat-fp32': dict(index='ivfflat', flat_storage='fp32'),
        'ivfflat-fx22': dict(index='ivfflat', flat_storage='fx22'),
        'ivfpq': dict(index='ivfpq'),
        'ivfpq-pre': dict(index='ivfpq', ann_window='pre'),
        'ivfpq-raw': dict(index='ivfpq', pq_by_residual=False),
        'ivfpq-refine': dict(index='ivfpq', refine_k=32),
        'winflat': dict(index='winflat'),
        'bf': dict(mode='bf'),
    },
    'unit': {'Da': dict(fragment_tolerance_unit='Da'),
             'ppm': dict(fragment_tolerance_unit='ppm', fragment_mz_tolerance=20.0)},
    'window': {'symmetric': dict(), 'asymmetric': dict(precursor_window_open=(-150.0, 500.0)),
               'isolation': dict()},
    'scorer': {'none': dict(), 'tdc': dict(device_fdr=True),
               'svm': dict(device_fdr=True, model='svm'),
               'rf': dict(device_fdr=True, model='rf', device_forest=True, forest_trees=16)},
}
AXIS_NAMES = tuple(AXES)
# the base the restatements of the single-feature tests are held against
FIRST = ('ivfflat-fp32', 'Da', 'symmetric', 'none')


def base_kwargs(base):
    """Config.open_search keywords of a base (a tuple of one value name per axis)."""
    kw = dict(ENGINE, device_decoys=True)
    for axis, value in zip(AXIS_NAMES, base):
        kw.update(AXES[axis][value])
    return kw


def accepted(kw):
    from ann_solo_amd.config import Config
    try:
        Config.open_search(**kw)
        return True
    except ValueError:
        return False


def pairs_of(base):
    return {((a, base[i]), (b, base[j])) for (i, a), (j, b) in itertools.combinations(enumerate(AXIS_NAMES), 2)}


def all_pairs():
    """Every pair of values of two different axes that ``Config`` accepts together."""
    out = set()
    for (i, a), (j, b) in itertools.combinations(enumerate(AXIS_NAMES), 2):
        for u in AXES[a]:
            for v in AXES[b]:
                if accepted(dict(ENGINE, **AXES[a][u], **AXES[b][v])):
                    out.add(((a, u), (b, v)))
    return out


_BASES = []


def bases():
    """A pairwise covering array, greedy: FIRST, then again and again the accepted base that covers the most
    pairs not covered so far (ties: the first in the axes' order). The two largest axes have 8 and 4 values, so
    no covering array has fewer than 32 rows; the greedy one has exactly that many."""
    if _BASES:
        return list(_BASES)
    todo = all_pairs()
    grid = [b for b in itertools.product(*(AXES[a] for a in AXIS_NAMES)) if accepted(base_kwargs(b))]
    out = [FIRST]
    todo -= pairs_of(FIRST)
    while todo:
        best = max(grid, key=lambda b: len(pairs_of(b) & todo))      # (max keeps the first of equals)
        assert pairs_of(best) & todo
        out.append(best)
        todo -= pairs_of(best)
    _BASES.extend(out)
    return list(out)


# ------------------------------------------------------------------------------------------------ the overlays
PRIMARY = ('charge', 'qrow', 'lib_row', 'score', 'q', 'open_level')      # and _peak_matches(i): on chimeric_rank 0
MOD_COLUMNS = ('mod_mass', 'mod_site_lo', 'mod_site_hi', 'mod_site_score', 'mod_site_margin', 'mod_site_gain')
ALT_COLUMNS = ('alt_lib_row', 'alt_score', 'delta_score')                # and alt_peak_matches(i, r)
STAT_COLUMNS = ('n_scored', 'expect')
CHIMERIC_COLUMNS = ('qrow', 'lib_row', 'score', 'q', 'chimeric_rank', 'explained_intensity')

# name -> dict(config: the keywords; needs: a predicate on the base; owns: the SSMTable columns only this overlay
# may change; rows: 'appended' when it adds rows behind the primary ones; route: how the run differs from
# search_packed on the packed queries). Everything an overlay does not own it must leave alone, to the byte.
OVERLAYS = {
    'score_stats': dict(config=dict(score_stats=True), owns=STAT_COLUMNS),
    'num_matches': dict(config=dict(num_matches=3), owns=ALT_COLUMNS),
    'distinct_matches': dict(config=dict(num_matches=3, distinct_matches=True), owns=ALT_COLUMNS),
    'localize_modifications': dict(config=dict(localize_modifications=True), owns=MOD_COLUMNS),
    'chimeric_search': dict(config=dict(chimeric_search=True), owns=(), rows='appended'),
    'device_qvalues': dict(config=dict(device_qvalues=True), owns=(), needs=lambda b: b[3] != 'none'),
    'device_groups': dict(config=dict(device_groups=True), owns=(), needs=lambda b: b[3] != 'none'),
    # (an MGF file has no field for an isolation window: the queries of that base cannot come from one)
    'device_mgf': dict(config=dict(device_mgf=True), owns=(), route='mgf', needs=lambda b: b[2] != 'isolation'),
    'device_library': dict(config=dict(device_library=True), owns=(), route='sptxt'),
    'batch_size': dict(config=dict(batch_size=97), owns=()),
}
# num_matches and distinct_matches set the same switch: 'all' takes the distinct one
EXCLUSIVE = {'num_matches': 'distinct_matches'}
# the Config switches every overlay needs one GPU for (asserted refused with num_gpus = 2)
SHARDED_REFUSED = ('score_stats', 'num_matches', 'distinct_matches', 'localize_modifications', 'chimeric_search',
                   'device_qvalues', 'device_groups')


def applicable(base):
    return [n for n, o in OVERLAYS.items() if o.get('needs', lambda b: True)(base)]


def overlay_sets(base, full=True, but_one=False):
    """The overlay sets of a base, as sorted tuples of names: none, all; ``full``: each applicable overlay alone;
    ``but_one``: all but one, for each. 'all' holds distinct_matches, not the plain num_matches beside it."""
    names = applicable(base)
    every = tuple(sorted(n for n in names if n not in EXCLUSIVE))
    out = [(), every]
    if full:
        out += [(n,) for n in names]
    if but_one:
        out += [tuple(m for m in every if m != n) for n in every]
        out.append(tuple(sorted(set(every) - {'distinct_matches'} | {'num_matches'})))
    return list(dict.fromkeys(out))


def overlay_kwargs(names):
    kw = {}
    for n in names:
        kw.update(OVERLAYS[n]['config'])
    return kw


def owned(names):
    out = set()
    for n in names:
        out.update(OVERLAYS[n]['owns'])
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def column_bytes(table, name, rows=None):
    a = np.ascontiguousarray(getattr(table, name) if rows is None else getattr(table, name)[rows])
    return a.dtype.str, a.shape, a.tobytes()


def assert_rows_equal(a, b, columns, rows_a=None, rows_b=None, peaks=True, what=''):
    """Columns ``columns`` of table a (rows ``rows_a``) and table b (``rows_b``) are the same bytes, and so are
    the rows' peak matches."""
    ra = np.arange(len(a)) if rows_a is None else np.asarray(rows_a)
    rb = np.arange(len(b)) if rows_b is None else np.asarray(rows_b)
    assert len(ra) == len(rb), (what, len(ra), len(rb))
    for name in columns:
        assert column_bytes(a, name, ra) == column_bytes(b, name, rb), (what, name)
    if peaks:
        for i, j in zip(ra, rb):
            assert np.array_equal(a._peak_matches(int(i)), b._peak_matches(int(j))), (what, 'peak matches', int(i))


# ------------------------------------------------------------------------------------------------ without a device
def host_packs(w, cfg):
    """The world packed on the host by the numpy preprocessing (tests/process_ref.py), for the oracle-backed
    engine: (library {charge: PackedSpectra.numpy() tuple}, library_meta, queries {charge: PackedSpectra},
    query_meta {charge: [record]}) -- query records as ``library_store.pack_queries`` writes them, queries without
    a charge entered at 2 and at 3, invalid spectra dropped."""
    from ann_solo_amd.packed import PackedSpectra
    from process_ref import numpy_process

    def process(s, z, max_peaks):
        return numpy_process(np.asarray(s.mz, np.float32), np.asarray(s.intensity, np.float32), float(s.precursor_mz), z,
                             cfg.min_mz, cfg.max_mz, cfg.remove_precursor, cfg.remove_precursor_tolerance,
                             cfg.min_intensity, max_peaks, cfg.scaling, cfg.min_peaks, cfg.min_mz_range, cfg.resolution)

    def pack(rows):     # rows: (mz, intensity, charge or None, precursor m/z, precursor charge)
        offs = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int32)
        chg = None if rows[0][2] is None else np.concatenate([r[2] for r in rows]).astype(np.uint8)
        return (offs, np.concatenate([r[0] for r in rows]).astype(np.float32),
                np.concatenate([r[1] for r in rows]).astype(np.float32), chg,
                np.array([r[3] for r in rows], np.float64), np.array([r[4] for r in rows], np.int32))
    lib_rows, lmeta = {}, {}
    for s in w['library']:
        z = int(s.precursor_charge)
        ok, mz, it, idx = process(s, z, cfg.max_peaks_used_library)
        assert ok
        chg = np.array([a.charge if a is not None else 0 for a in s.annotation], np.uint8)[idx]
        lib_rows.setdefault(z, []).append((mz, it, chg, float(s.precursor_mz), z))
        lmeta.setdefault(z, []).append(dict(identifier=s.identifier, peptide=s.peptide, is_decoy=False,
                                            precursor_mz=float(np.float32(s.precursor_mz))))
    q_rows, qmeta = {}, {}
    for pos, s in enumerate(w['queries']):
        for z in ([s.precursor_charge] if s.precursor_charge is not None else [2, 3]):
            ok, mz, it, _ = process(s, z, cfg.max_peaks_used)
            if not ok:
                continue
            q_rows.setdefault(z, []).append((mz, it, None, float(s.precursor_mz), z))
            qmeta.setdefault(z, []).append(dict(identifier=s.identifier, index=s.index, retention_time=s.retention_time,
                                                precursor_charge=z, precursor_mz=float(s.precursor_mz)))
    return ({z: pack(r) for z, r in lib_rows.items()}, lmeta,
            {z: PackedSpectra.from_numpy(*pack(r)) for z, r in q_rows.items()}, qmeta)


def cosines_of(table, rows, queries, partitions):
    """The cosine over the peak matches the table holds for ``rows`` (float64, summed in pair order):
    ``queries[charge]`` and ``partitions[charge]`` are ``PackedSpectra.numpy()`` tuples. What ``table.score`` must
    be for a row of a level without a learned scorer -- if its peak matches are its own."""
    out = np.empty(len(rows))
    for k, i in enumerate(rows):
        z = int(table.charge[i])
        (qo, _, qi, *_), (lo, _, li, *_) = queries[z], partitions[z]
        pm = table._peak_matches(int(i))
        a, b = int(qo[table.qrow[i]]), int(lo[table.lib_row[i]])
        assert len(pm) == 0 or (pm[:, 0].max() < qo[table.qrow[i] + 1] - a and pm[:, 1].max() < lo[table.lib_row[i] + 1] - b)
        out[k] = float(np.sum(qi[a + pm[:, 0]].astype(np.float64) * li[b + pm[:, 1]].astype(np.float64)))
    return out
