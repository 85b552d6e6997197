"""What reading an mzXML query file costs, on the device and on the host: a synthetic file of 10^5 MS2 scans of about
100 peaks (64-bit zlib streams), ten of them nested in each MS1 scan with a profile-sized stream of its own, in the
layout ReAdW writes (tests/mzxml_cases.py), is read

  * by ``mzxml.read_mzxml_packed`` -- tags parsed and streams decoded by the kernels of csrc/mzxml.hip --, split into
    reading the file, the parse (upload, kernels, identifiers and columns on the host) and the preprocessing with
    the meta records; the decode kernel's device time alone comes from the library's stage profile
    (``mzxml_decode``), in calls of their own;
  * by ``library_store.pack_queries`` over ``tests/mzxml_ref.read_mzxml`` -- the same dialect in plain Python
    (ElementTree, base64, zlib, numpy) on one core: the only CPU baseline at hand, and not pyteomics.

One warm-up, five timed calls each: median, range and every time. Writes profiles/mzxml_cost.json. Records, not
thresholds: no rate was promised.

    python scripts/mzxml_cost.py [--out profiles/mzxml_cost.json] [--scans 100000] [--peaks 100] [--host_repeats 5]
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
DISTINCT = 1000          # distinct MS2 scans; the file repeats them under new scan numbers
PROFILE_POINTS = 4000    # pairs of an MS1 profile stream
PER_SURVEY = 10          # MS2 scans nested in one MS1 scan


def synthetic_mzxml(n_scans: int, n_peaks: int, seed: int = 7) -> bytes:
    import mzxml_cases as XC
    rng = np.random.default_rng(seed)
    grid = np.linspace(300.0, 1700.0, PROFILE_POINTS)
    tile, k = [], 0
    distinct = min(DISTINCT, n_scans)
    for g in range(0, distinct, PER_SURVEY):
        survey = k
        k += 1
        kids = []
        for i in range(g, min(g + PER_SURVEY, distinct)):
            n = int(rng.integers(n_peaks - 20, n_peaks + 21))
            mz = np.sort(np.round(rng.uniform(100.0, 1900.0, n), 5))
            kids.append(XC.scan('@%04d' % k, mz, np.round(rng.lognormal(6.0, 1.5, n), 2), f64=True, z=True,
                                rt='PT%.4fS' % rng.uniform(0.0, 7200.0), pmz='%.5f' % rng.uniform(350.0, 1400.0),
                                charge=int(rng.integers(2, 5)) if i % 8 else None, pad='      '))
            k += 1
        tile.append(XC.scan('@%04d' % survey, grid, rng.lognormal(8.0, 2.0, PROFILE_POINTS), level=1, z=True,
                            rt='PT%.4fS' % rng.uniform(0.0, 7200.0), children=kids))
    tile = ''.join(tile)
    body = ''.join(tile.replace('@', str(t + 1)) for t in range(n_scans // distinct))
    return (XC.HEAD % body.count('<scan ') + body + XC.TAIL + XC.INDEX + '</mzXML>\n').encode()


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


def stage_ms(L, stage):
    ms, n = C.c_double(0.0), C.c_int64(0)
    L.asl_profile_get(stage.encode(), C.byref(ms), C.byref(n))
    return ms.value, n.value


def main():
    import torch
    import mzxml_ref
    from ann_solo_amd import _lib, mzxml
    from ann_solo_amd.config import Config
    from ann_solo_amd.library_store import pack_queries
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mzxml_cost.json'))
    ap.add_argument('--scans', type=int, default=100000)
    ap.add_argument('--peaks', type=int, default=100)
    ap.add_argument('--host_repeats', type=int, default=REPEATS)
    args = ap.parse_args()
    cfg, dev = Config(), 'cuda:0'
    data = synthetic_mzxml(args.scans, args.peaks)
    n_bytes = len(data)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'synthetic.mzXML')
        with open(path, 'wb') as f:
            f.write(data)
        del data
        runs = []

        def device():
            st = {}
            out = mzxml.read_mzxml_packed(path, cfg, dev, stats=st)
            torch.cuda.synchronize()
            runs.append(st)
            return out
        (d_packs, d_meta), t_dev = timed(device)
        runs = runs[1:]
        keys = ('chunks', 'grown', 'n_lines', 'n_spectra', 'n_peaks', 'n_sorted', 'n_skipped_level', 'n_skipped_id',
                'n_arrays', 'n_zlib', 'n_nested')
        doc_dev = dict(read_mzxml_packed=summary(t_dev, n_bytes),
                       read_file=summary([r['read_s'] for r in runs], n_bytes),
                       parse=summary([r['parse_s'] for r in runs], n_bytes),
                       preprocess_and_meta=summary([r['process_s'] for r in runs], n_bytes),
                       counts={k: runs[0][k] for k in keys})
        # the decode kernel alone: device time between events, in calls of their own
        L = _lib.lib()
        decode, fill = [], []
        for _ in range(REPEATS + 1):
            L.asl_profile_reset()
            L.asl_profile_enable(1)
            mzxml.read_mzxml_packed(path, cfg, dev)
            torch.cuda.synchronize()
            decode.append(stage_ms(L, 'mzxml_decode')[0] / 1e3)
            fill.append((stage_ms(L, 'mzxml_fill')[0] + stage_ms(L, 'mzxml_measure')[0]) / 1e3)
            L.asl_profile_enable(0)
        doc_dev['decode_kernel_device_time'] = summary(decode[1:], n_bytes)
        doc_dev['measure_and_fill_device_time'] = summary(fill[1:], n_bytes)
        print(json.dumps(doc_dev), flush=True)
        # the same dialect in Python, one core
        torch.set_num_threads(1)
        split = []

        def host():
            t0 = time.perf_counter()
            objs = mzxml_ref.read_mzxml(path)
            t1 = time.perf_counter()
            out = pack_queries(objs, cfg, dev)
            torch.cuda.synchronize()
            split.append((t1 - t0, time.perf_counter() - t1))
            return out
        (h_packs, h_meta), t_host = timed(host, args.host_repeats)
        split = split[1:]
        doc_host = dict(pack_queries_over_mzxml_ref=summary(t_host, n_bytes),
                        parse=summary([s[0] for s in split], n_bytes),
                        pack_queries=summary([s[1] for s in split], n_bytes), repeats=args.host_repeats)
        print(json.dumps(doc_host), flush=True)
        same = d_meta == h_meta and list(d_packs) == list(h_packs) and all(
            a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            for z in h_packs for a, b in zip(d_packs[z]._tensors(), h_packs[z]._tensors()))
    doc = dict(what='wall time in seconds of one call on a file in the page cache, synchronised; one warm-up and five '
                    'timed calls each. device: mzxml.read_mzxml_packed(path) and its three parts as the reader times '
                    'them (read_file: the file into host memory; parse: upload, kernels, identifiers and columns on '
                    'the host; preprocess_and_meta: process_spectra, the per-charge gathers, the copies to the host '
                    'and the meta records); decode_kernel_device_time: the launches of the decode kernel between '
                    'device events, per call. host: library_store.pack_queries over tests/mzxml_ref.read_mzxml '
                    '(ElementTree, base64, zlib, numpy), one core; pyteomics is not a dependency and was not '
                    'measured.',
               file=dict(bytes=n_bytes, ms2_scans=doc_dev['counts']['n_spectra'],
                         other_scans=doc_dev['counts']['n_skipped_level'], peaks_per_scan='%d +- 20' % args.peaks,
                         streams='64-bit float pairs, zlib level 6', ms1_profile_points=PROFILE_POINTS,
                         ms2_per_ms1=PER_SURVEY, distinct_scans=min(DISTINCT, args.scans)),
               decode_shape='one thread per stream, windows in global scratch; the wave-per-stream shape is not built',
               repeats=REPEATS, gpu=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)),
               device=doc_dev, host=doc_host, same_result=bool(same),
               host_over_device_median=round(float(np.median(t_host)) / float(np.median(t_dev)), 1),
               note='No threshold was set.')
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: doc[k] for k in ('same_result', 'host_over_device_median')}))


if __name__ == '__main__':
    main()
