"""Writes tests/golden/decoy_kat.json: the known answer the reference ships for its decoy generator
(/root/reference/src/tests/decoy_generator_test.py), as data. Only numbers and names are taken from that
file -- the four arrays (target m/z and intensity, expected decoy m/z and intensity), the two peptide
strings, the precursor m/z and charge and the tolerance (10 ppm) -- by pattern, nothing is executed.

    python tests/golden/make_decoy_kat.py [path of decoy_generator_test.py]

The test's mocked position mapping is not a permutation that produces its decoy sequence (it is only
right at the two C's), so ``perm`` is derived from the two sequences: decoy residue i is the first unused
target residue with the same letter and modification; equal residues are interchangeable."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NUM = r'[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?'


def tokens(peptide):
    return re.findall(r'[A-Z](?:\[[^\]]*\])?', peptide)


def main(path):
    text = open(path).read()
    arrays = [[float(v) for v in re.findall(NUM, body)]
              for body in re.findall(r'np\.asarray\(\s*\[(.*?)\]', text, flags=re.S)]
    assert len(arrays) == 4 and len({len(a) for a in arrays}) == 1, [len(a) for a in arrays]
    spectra = re.findall(r'MsmsSpectrum\("([^"]+)",\s*(' + NUM + r'),\s*(\d+)', text)
    assert len(spectra) == 2 and spectra[0][1:] == spectra[1][1:], spectra
    tol = re.search(r'"fragment_mz_tolerance":\s*(' + NUM + r')', text).group(1)
    unit = re.search(r'"fragment_tol_mode":\s*\'(\w+)\'', text).group(1)
    target, decoy = tokens(spectra[0][0]), tokens(spectra[1][0])
    used, perm = set(), []
    for tok in decoy:
        i = next(i for i, t in enumerate(target) if t == tok and i not in used)
        used.add(i)
        perm.append(i)
    out = dict(peptide=spectra[0][0], decoy_peptide=spectra[1][0], perm=perm,
               precursor_mz=float(spectra[0][1]), precursor_charge=int(spectra[0][2]),
               tolerance=float(tol), unit=unit, mz=arrays[0], intensity=arrays[1], decoy_mz=arrays[2],
               decoy_intensity=arrays[3])
    with open(os.path.join(HERE, 'decoy_kat.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/root/reference/src/tests/decoy_generator_test.py')
