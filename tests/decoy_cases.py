"""Random peptides and raw spectra for the decoy tests: a spectrum is built from its own peptide's
theoretical fragments (with a mass error around the tolerance, so that some fall just outside) plus noise
peaks, ascending float32 m/z."""
import numpy as np

import decoy_ref as R

LETTERS = 'GASPVTCLINDQKEMHFRYW'


def random_peptide(rng, L, mod_p=0.15, negative=False, light=False):
    """A peptide string of L residues; ``negative``: one residue carries a negative mass difference;
    ``light``: one residue is modified down to under 1e-3 Da and one below zero (ladders that do not
    rise steadily: the kernel's exhaustive branch)."""
    from ann_solo_amd.decoy_generator import RESIDUE_MASS
    seq = [LETTERS[i] for i in rng.integers(0, len(LETTERS), L)]
    if rng.random() < 0.8:
        seq[-1] = 'KR'[int(rng.integers(0, 2))]
    out = []
    special = {}
    if negative:
        special[int(rng.integers(0, L))] = '[-18.010565]'
    if light and L >= 3:
        i, j = rng.choice(L, 2, replace=False)
        special[int(i)] = '[%.6f]' % (-RESIDUE_MASS[seq[i]] + 2.5e-4)
        special[int(j)] = '[%.6f]' % (-RESIDUE_MASS[seq[j]] - 3.0)
    for i, a in enumerate(seq):
        tag = special.get(i, '')
        if not tag and rng.random() < mod_p:
            tag = ('[Oxidation]', '[+79.966331]', '[Carbamidomethyl]', '[0.984016]')[int(rng.integers(0, 4))]
        out.append(a + tag)
    return ''.join(out)


def make_case(rng, L, Z, n_peaks, tol, unit, nterm=0.0, cterm=0.0, negative=False, light=False,
              identity=False, frac=0.6):
    from ann_solo_amd import decoy_generator as dg
    text = random_peptide(rng, L, negative=negative, light=light)
    pep = dg.parse_peptide(text)
    masses = pep.masses
    _, perm = dg.shuffle(pep.sequence, rng)
    if identity:
        perm = list(range(L))
    zmax = max(1, Z - 1)
    ft, fn, fz, fl, base = R.fragment_table(masses, nterm, cterm, zmax)
    theo = R.theo_of(base, fl, fz)
    theo = theo[(theo > 40.0) & (theo < 4000.0)]
    n_frag = min(int(frac * n_peaks), len(theo)) if len(theo) else 0
    t = rng.choice(theo, n_frag, replace=len(theo) < n_frag) if n_frag else np.zeros(0)
    reach = tol if unit == 'Da' else tol * 1e-6 * t
    mz = np.concatenate((t + rng.uniform(-1.3, 1.3, n_frag) * reach,
                         rng.uniform(50.0, max(300.0, float(masses.sum())), n_peaks - n_frag)))
    mz = np.sort(mz.astype(np.float32))
    inten = rng.lognormal(0.0, 1.2, n_peaks).astype(np.float32)
    return dict(peptide=text, masses=masses, perm=np.asarray(perm, np.int32), nterm=float(nterm),
                cterm=float(cterm), zmax=zmax, charge=int(Z), mz=mz, intensity=inten, L=L)


def pack_cases(cases):
    """(PackedSpectra on the host, seq_offsets, residue_mass, perm, nterm, cterm, zmax)."""
    from ann_solo_amd.packed import PackedSpectra
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if len(xs) else np.zeros(0, dt)
    off = np.concatenate(([0], np.cumsum([len(c['mz']) for c in cases]))).astype(np.int32)
    seq = np.concatenate(([0], np.cumsum([c['L'] for c in cases]))).astype(np.int32)
    raw = PackedSpectra.from_numpy(off, cat([c['mz'] for c in cases], np.float32),
                                   cat([c['intensity'] for c in cases], np.float32), None,
                                   np.full(len(cases), 500.0), np.asarray([c['charge'] for c in cases], np.int32),
                                   'cpu', list(range(len(cases))))
    return (raw, seq, cat([c['masses'] for c in cases], np.float64), cat([c['perm'] for c in cases], np.int32),
            np.asarray([c['nterm'] for c in cases], np.float64), np.asarray([c['cterm'] for c in cases], np.float64),
            np.asarray([c['zmax'] for c in cases], np.int32))


def reference(cases, tol, unit):
    return [R.decoy_ref(c['mz'], c['intensity'], c['masses'], c['perm'], c['nterm'], c['cterm'], c['zmax'],
                        tol, unit) for c in cases]


KEYS = ('src', 'charge', 'ann_type', 'ann_n', 'ann_z', 'ann_loss')


def assert_same(out, refs, offsets, what=''):
    """Bit for bit: float32 m/z bits, intensities, src, decoy charge and the four annotation columns."""
    for s, r in enumerate(refs):
        a, b = int(offsets[s]), int(offsets[s + 1])
        assert np.array_equal(out['mz'][a:b].view(np.uint32), r['mz'].view(np.uint32)), (what, s, 'mz')
        assert np.array_equal(out['intensity'][a:b].view(np.uint32), r['intensity'].view(np.uint32)), (what, s)
        for k in KEYS:
            assert np.array_equal(out[k][a:b], r[k]), (what, s, k)
