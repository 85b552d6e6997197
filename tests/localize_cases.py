"""Case builders for the localisation tests: peptides (``decoy_cases.random_peptide``) with query spectra
built from their own plain and shifted b / y fragments, packing for ``localize_batch`` and the bit-for-bit
comparison with ``localize_ref``."""
import numpy as np

import decoy_cases as DC
import localize_ref as R

DELTAS = (15.994915, 79.966331, -17.026549, 42.010565, 203.079373)
SITE_KEYS = ('site_score', 'site_count')
SSM_KEYS = ('best_lo', 'best_hi', 'n_best', 'best_count', 'best_score', 'runner_score', 'none_score')


def parse(text):
    from ann_solo_amd.decoy_generator import parse_peptide
    return parse_peptide(text)


def case(masses, mz, intensity, delta, zmax=1, nterm=0.0, cterm=0.0, **extra):
    order = np.argsort(np.asarray(mz, np.float32), kind='stable')
    return dict(masses=np.asarray(masses, np.float64), L=len(masses), nterm=float(nterm), cterm=float(cterm),
                zmax=int(zmax), delta=float(delta), mz=np.asarray(mz, np.float32)[order],
                intensity=np.asarray(intensity, np.float32)[order], **extra)


def ladder_mz(masses, site, delta, nterm=0.0, cterm=0.0):
    """Singly charged b_1 .. b_{L-1}, y_1 .. y_{L-1} (float64) of the peptide with ``delta`` on residue
    ``site``: ``(b, y)``, element k - 1 is fragment k."""
    m = np.array(masses, np.float64)
    m[site] += delta
    P, S = R.ladders(m, nterm, cterm)
    return P[1:-1] + R.PROTON, S[1:-1] + R.H2O + R.PROTON


def planted_case(rng, L, delta, site, sigma=0.003, drop_b=(), drop_y=()):
    """A complete singly charged b / y ladder of a random peptide carrying ``delta`` on ``site`` (minus
    the fragments ``drop_b`` / ``drop_y``), m/z jittered by N(0, sigma), float32; charge up to 2."""
    text = DC.random_peptide(rng, L)
    pep = parse(text)
    b, y = ladder_mz(pep.masses, site, delta)
    keep_b = [k for k in range(1, L) if k not in drop_b]
    keep_y = [k for k in range(1, L) if k not in drop_y]
    mz = np.concatenate((b[[k - 1 for k in keep_b]], y[[k - 1 for k in keep_y]]))
    mz = mz + rng.normal(0.0, sigma, len(mz)) if sigma else mz
    inten = rng.lognormal(0.0, 0.5, len(mz))
    return case(pep.masses, mz, inten, delta, zmax=2, peptide=text, site=site)


def random_case(rng, L, zmax, n_peaks, tol, unit, delta, nterm=0.0, cterm=0.0, frac=0.6):
    """``n_peaks`` peaks: plain and shifted fragments of a random peptide with an m/z error around the
    tolerance (some fall just outside), the rest noise."""
    pep = parse(DC.random_peptide(rng, L))
    theo = R.fragment_theo(pep.masses, nterm, cterm, delta, zmax)[:, 1:].reshape(-1)
    n_frag = min(int(frac * n_peaks), len(theo))
    t = rng.choice(theo, n_frag, replace=False) if n_frag else np.zeros(0)
    reach = np.full(n_frag, tol) if unit == 'Da' else tol * 1e-6 * np.abs(t)
    hi = max(300.0, float(pep.masses.sum()))
    mz = np.concatenate((t + rng.uniform(-1.3, 1.3, n_frag) * reach, rng.uniform(-5.0, hi, n_peaks - n_frag)))
    inten = np.round(rng.lognormal(0.0, 1.2, n_peaks), 1)      # coarse: equal intensities do occur
    return case(pep.masses, mz, inten, delta, zmax, nterm, cterm)


def pack_cases(cases, device='cpu'):
    """``(PackedSpectra, seq_offsets, residue_mass, nterm, cterm, zmax, delta)``: ``localize_batch``'s
    arguments up to the tolerance."""
    from ann_solo_amd.packed import PackedSpectra
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if len(xs) else np.zeros(0, dt)
    off = np.concatenate(([0], np.cumsum([len(c['mz']) for c in cases]))).astype(np.int32)
    seq = np.concatenate(([0], np.cumsum([c['L'] for c in cases]))).astype(np.int32)
    q = PackedSpectra.from_numpy(off, cat([c['mz'] for c in cases], np.float32),
                                 cat([c['intensity'] for c in cases], np.float32), None,
                                 np.full(len(cases), 500.0), np.full(len(cases), 2, np.int32), device,
                                 list(range(len(cases))))
    col = lambda k, dt: np.asarray([c[k] for c in cases], dt)
    return (q, seq, cat([c['masses'] for c in cases], np.float64), col('nterm', np.float64),
            col('cterm', np.float64), col('zmax', np.int32), col('delta', np.float64))


def reference(cases, tol, unit):
    return [R.localize_ref(c['mz'], c['intensity'], c['masses'], c['nterm'], c['cterm'], c['zmax'], c['delta'],
                           tol, unit) for c in cases]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(out, refs, seq, what=''):
    """Every output against the reference: integers equal, scores as uint64 views."""
    out = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)) for k, v in out.items()}
    for s, r in enumerate(refs):
        a, b = int(seq[s]), int(seq[s + 1])
        assert np.array_equal(bits(out['site_score'][a:b]), bits(r['site_score'])), (what, s, 'site_score')
        assert np.array_equal(out['site_count'][a:b], r['site_count']), (what, s, 'site_count')
        for k in SSM_KEYS:
            if k.endswith('score'):
                assert bits(out[k][s:s + 1])[0] == bits([r[k]])[0], (what, s, k, out[k][s], r[k])
            else:
                assert int(out[k][s]) == r[k], (what, s, k, out[k][s], r[k])
