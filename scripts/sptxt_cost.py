"""What reading a .sptxt spectral library costs, on the device and on the host: a synthetic file of 10^5 records of
about 100 annotated peaks, with SpectraST-like Comment lines of about 600 bytes, is read

  * by ``sptxt.build_store`` (what ``sptxt.read_library`` runs when no packed store is cached) -- the text parsed
    by the kernels of csrc/sptxt.hip, split into reading the file, the parse (upload, kernels, the host's peptide
    strings and record checks) and the preprocessing; one more call with the library's stage profile on lists the
    device time of every kernel group;
  * by ``library_store.build_library_store`` over ``tests/sptxt_ref.read_sptxt`` -- the same dialect in plain Python
    on one core. It is the only CPU baseline at hand and it is NOT the reference's code, which needs pyteomics,
    spectrum_utils, h5py and FAISS and writes every spectrum to HDF5 and reads it back on top of a parse like this.

One warm-up and five timed calls of the device reader, two timed calls of the host statement (minutes each):
median, range and every time. Writes profiles/sptxt_cost.json. Records, not
thresholds: no ratio was fixed in advance.

    python scripts/sptxt_cost.py [--out profiles/sptxt_cost.json] [--records 100000] [--peaks 100]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

REPEATS = 5
DISTINCT = 1000          # distinct records; the file repeats them (identifiers are ordinals)
FLAGSHIP = 2_100_000     # library spectra of the flagship workload
STAGES = ('sptxt_measure', 'sptxt_starts', 'sptxt_classify', 'sptxt_state', 'sptxt_parse', 'sptxt_counts',
          'sptxt_resolve', 'sptxt_fill', 'sptxt_fill_lines', 'sptxt_fill_records', 'mgf_sort')


def synthetic_sptxt(n_records: int, n_peaks: int, seed: int = 7) -> bytes:
    import sptxt_cases as SC
    rng = np.random.default_rng(seed)
    pad = ' '.join('Field%d=%s' % (k, 'x' * 12) for k in range(24))          # about 450 bytes more of Comment
    records = []
    for i in range(min(DISTINCT, n_records)):
        k = int(rng.integers(n_peaks - 20, n_peaks + 21))
        records.append(SC.record(rng, charge=int(rng.integers(2, 5)), n_peaks=k, comment_extra=' ' + pad,
                                 decoy='comment' if i % 10 == 0 else None))
    tile = ''.join(records)
    return (tile * (n_records // len(records))).encode()


def timed(fn, repeats=REPEATS, warm_up=True):
    if warm_up:
        fn()                                 # allocations, code objects, caches
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


def main():
    import torch
    import sptxt_ref
    from fake_reader import FakeReader
    from ann_solo_amd import _lib, sptxt
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import build_library_store
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sptxt_cost.json'))
    ap.add_argument('--records', type=int, default=100000)
    ap.add_argument('--peaks', type=int, default=100)
    args = ap.parse_args()
    cfg, dev = Config(), 'cuda:0'
    data = synthetic_sptxt(args.records, args.peaks)
    n_bytes, n_lines = len(data), data.count(b'\n')
    comment = np.mean([len(l) for l in data[:1 << 20].split(b'\n') if l.startswith(b'Comment:')])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'synthetic.sptxt')
        with open(path, 'wb') as f:
            f.write(data)
        del data
        runs = []

        def device():
            st = {}
            out = sptxt.build_store(path, cfg, dev, stats=st)
            torch.cuda.synchronize()
            runs.append(st)
            return out
        d_store, t_dev = timed(device)
        runs = runs[1:]
        L = _lib.lib()
        L.asl_profile_reset()
        L.asl_profile_enable(1)
        device()
        L.asl_profile_enable(0)
        kernels = {}
        for s in STAGES:
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            L.asl_profile_get(s.encode(), C.byref(ms), C.byref(cnt))
            kernels[s] = dict(ms=round(ms.value, 3), scopes=int(cnt.value))
        doc_dev = dict(build_store=summary(t_dev, n_bytes),
                       read_file=summary([r['read_s'] for r in runs], n_bytes),
                       parse=summary([r['parse_s'] for r in runs], n_bytes),
                       preprocess=summary([r['process_s'] for r in runs], n_bytes),
                       counts={k: runs[0][k] for k in ('chunks', 'grown', 'n_lines', 'n_records', 'n_peaks',
                                                       'n_deferred', 'n_sorted')},
                       device_ms_of_one_profiled_call=kernels)
        print(json.dumps(doc_dev), flush=True)
        # the same dialect in Python, one core
        torch.set_num_threads(1)
        split = []

        def host():
            t0 = time.perf_counter()
            objs = sptxt_ref.read_sptxt(path)
            t1 = time.perf_counter()
            out = build_library_store(FakeReader(objs), cfg, dev)
            torch.cuda.synchronize()
            split.append((t1 - t0, time.perf_counter() - t1))
            return out
        h_store, t_host = timed(host, repeats=2, warm_up=False)     # (minutes: the device calls warmed the kernels)
        doc_host = dict(build_library_store_over_sptxt_ref=summary(t_host, n_bytes),
                        parse=summary([s[0] for s in split], n_bytes),
                        build_library_store=summary([s[1] for s in split], n_bytes), repeats=2)
        print(json.dumps(doc_host), flush=True)
        same = (d_store.meta == h_store.meta and d_store.ranges == h_store.ranges and
                d_store.valid.tobytes() == h_store.valid.tobytes() and
                all(a.numpy().tobytes() == b.numpy().tobytes()
                    for a, b in zip(d_store.spectra._tensors(), h_store.spectra._tensors())))
    med_dev, med_host = float(np.median(t_dev)), float(np.median(t_host))
    scale = FLAGSHIP / args.records
    doc = dict(what='wall time in seconds of one call on a file in the page cache, synchronised; one warm-up and five '
                    'timed calls of the device reader, two timed calls of the host statement. device: '
                    'sptxt.build_store(path) and its three parts as the reader times them (read_file: the file into '
                    'host memory; parse: upload, kernels, deferred numerals, peptide strings and record checks on the '
                    'host; preprocess: process_spectra and the copies to the host), and the device time of each '
                    'kernel group in one more call (asl_profile_get; sptxt_measure and sptxt_fill contain the groups '
                    'listed under them and their synchronisations). One thread walks each line, the Comment lines '
                    'included: sptxt_parse is where that shows. host: library_store.build_library_store over '
                    'tests/sptxt_ref.read_sptxt, one core: the only CPU baseline at hand, and not the reference\'s code.',
               file=dict(bytes=n_bytes, lines=n_lines, records=args.records,
                         peaks_per_record='%d +- 20' % args.peaks, distinct_records=min(DISTINCT, args.records),
                         mean_comment_line_bytes=round(float(comment))),
               repeats=REPEATS, gpu=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)),
               device=doc_dev, host=doc_host, same_result=bool(same),
               host_over_device_median=round(med_host / med_dev, 1),
               extrapolation=dict(records=FLAGSHIP, bytes=round(n_bytes * scale),
                                  device_s=round(med_dev * scale, 1), host_s=round(med_host * scale, 1),
                                  note='an extrapolation, not a measurement: the medians above times %.0f, assuming '
                                       'time linear in the file size (the reader works chunk by chunk) and the file '
                                       'in the page cache' % scale),
               note='No threshold was set.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: doc[k] for k in ('same_result', 'host_over_device_median')}))


if __name__ == '__main__':
    main()
