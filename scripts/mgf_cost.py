"""What reading an MGF query file costs, on the device and on the host: a synthetic file of 10^5 spectra of about
100 peaks (numerals of at most 15 digits, so the device defers none) is read

  * by ``mgf.read_mgf_packed`` -- the text parsed by the kernels of csrc/mgf.hip, split into reading the file,
    the parse (upload, kernels, the host's identifiers and columns) and the preprocessing with the meta records;
  * by ``library_store.pack_queries`` over ``tests/mgf_ref.read_mgf`` -- the same dialect in plain Python on one
    core, the stand-in for the reference's reader, which is not a dependency of this project;
  * by ``pack_queries`` over pyteomics' ``mgf.MGF`` shaped as the reference's ``read_mgf`` shapes it, when
    pyteomics imports.

One warm-up, five timed calls each: median, range and every time. Writes profiles/mgf_cost.json. Records, not
thresholds: no ratio was fixed in advance.

    python scripts/mgf_cost.py [--out profiles/mgf_cost.json] [--spectra 100000] [--peaks 100]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REPEATS = 5
DISTINCT = 1000          # distinct spectra; the file repeats them under new titles


def synthetic_mgf(n_spectra: int, n_peaks: int, seed: int = 7) -> bytes:
    rng = np.random.default_rng(seed)
    blocks = []
    for i in range(min(DISTINCT, n_spectra)):
        k = int(rng.integers(n_peaks - 20, n_peaks + 21))
        mz = np.sort(rng.uniform(100.0, 1900.0, k))
        it = rng.lognormal(6.0, 1.5, k)
        head = ['BEGIN IONS', 'TITLE=run.@.%d' % i, 'PEPMASS=%.5f %.1f' % (rng.uniform(350.0, 1400.0), it.sum()),
                'RTINSECONDS=%.3f' % rng.uniform(0.0, 7200.0)]
        if i % 8:
            head.append('CHARGE=%d+' % rng.integers(2, 5))
        blocks.append('\n'.join(head + ['%.5f %.2f' % p for p in zip(mz, it)] + ['END IONS', '']))
    tile = '\n'.join(blocks)
    out = [tile.replace('@', str(t)) for t in range(n_spectra // len(blocks))]
    return '\n'.join(out).encode()


def timed(fn, repeats=REPEATS):
    fn()                                     # warm-up: allocations, code objects, caches
    times, out = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, times


def summary(times, n_bytes):
    med = float(np.median(times))
    return dict(median_s=round(med, 4), min_s=round(min(times), 4), max_s=round(max(times), 4),
                all_s=[round(t, 4) for t in times], bytes_per_s=round(n_bytes / med))


def pyteomics_reader(path):
    from pyteomics import mgf as pmgf
    with pmgf.MGF(path) as f:
        for i, s in enumerate(f, 1):
            p = s['params']
            yield SimpleNamespace(identifier=p['title'] if 'title' in p else p['scan'],
                                  precursor_mz=float(p['pepmass'][0]),
                                  precursor_charge=int(p['charge'][0]) if 'charge' in p else None,
                                  mz=s['m/z array'], intensity=s['intensity array'],
                                  retention_time=float(p['rtinseconds']) if 'rtinseconds' in p else None, index=i)


def main():
    import torch
    import mgf_ref
    from ann_solo_amd import mgf
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mgf_cost.json'))
    ap.add_argument('--spectra', type=int, default=100000)
    ap.add_argument('--peaks', type=int, default=100)
    args = ap.parse_args()
    cfg, dev = Config(), 'cuda:0'
    data = synthetic_mgf(args.spectra, args.peaks)
    n_bytes = len(data)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'synthetic.mgf')
        with open(path, 'wb') as f:
            f.write(data)
        del data
        # the device reader
        runs = []

        def device():
            st = {}
            out = mgf.read_mgf_packed(path, cfg, dev, stats=st)
            torch.cuda.synchronize()
            runs.append(st)
            return out
        (d_packs, d_meta), t_dev = timed(device)
        runs = runs[1:]
        doc_dev = dict(read_mgf_packed=summary(t_dev, n_bytes),
                       read_file=summary([r['read_s'] for r in runs], n_bytes),
                       parse=summary([r['parse_s'] for r in runs], n_bytes),
                       preprocess_and_meta=summary([r['process_s'] for r in runs], n_bytes),
                       counts={k: runs[0][k] for k in ('chunks', 'grown', 'n_lines', 'n_spectra', 'n_peaks',
                                                       'n_deferred', 'n_sorted')})
        print(json.dumps(doc_dev), flush=True)
        # the same dialect in Python, one core
        torch.set_num_threads(1)
        split = []

        def host():
            t0 = time.perf_counter()
            objs = mgf_ref.read_mgf(path)
            t1 = time.perf_counter()
            out = pack_queries(objs, cfg, dev)
            torch.cuda.synchronize()
            split.append((t1 - t0, time.perf_counter() - t1))
            return out
        (h_packs, h_meta), t_host = timed(host)
        split = split[1:]
        doc_host = dict(pack_queries_over_mgf_ref=summary(t_host, n_bytes),
                        parse=summary([s[0] for s in split], n_bytes),
                        pack_queries=summary([s[1] for s in split], n_bytes))
        print(json.dumps(doc_host), flush=True)
        same = d_meta == h_meta and list(d_packs) == list(h_packs) and all(
            a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            for z in h_packs for a, b in zip(d_packs[z]._tensors(), h_packs[z]._tensors()))
        # pyteomics, when it is there
        try:
            import pyteomics  # noqa: F401
            (p_packs, p_meta), t_py = timed(lambda: pack_queries(pyteomics_reader(path), cfg, dev))
            doc_py = dict(pack_queries_over_pyteomics=summary(t_py, n_bytes), same_meta=bool(p_meta == h_meta))
        except ImportError:
            doc_py = 'pyteomics is not importable: not measured'
    doc = dict(what='wall time in seconds of one call on a file in the page cache, synchronised; one warm-up and five '
                    'timed calls each. device: mgf.read_mgf_packed(path) and its three parts as the reader times them '
                    '(read_file: the file into host memory; parse: upload, kernels, deferred numerals, identifiers '
                    'and columns on the host; '
                    'preprocess_and_meta: process_spectra, the per-charge gathers, the copies to the host and the meta '
                    'records). host: library_store.pack_queries over tests/mgf_ref.read_mgf, one core.',
               file=dict(bytes=n_bytes, spectra=args.spectra, peaks_per_spectrum='%d +- 20' % args.peaks,
                         distinct_spectra=min(DISTINCT, args.spectra), numerals='at most 15 digits'),
               repeats=REPEATS, gpu=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)),
               device=doc_dev, host=doc_host, pyteomics=doc_py, same_result=bool(same),
               host_over_device_median=round(float(np.median(t_host)) / float(np.median(t_dev)), 1),
               note='No threshold was set.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: doc[k] for k in ('same_result', 'host_over_device_median')}))


if __name__ == '__main__':
    main()
