"""SpectraST ``.sptxt`` libraries read on the device (``Config.device_library``; DESIGN.md 3 "Library files").

``read_library(filename, config, device)`` returns a reader object that holds the ``LibraryStore``
``library_store.build_library_store`` makes of the same file read record by record in Python -- the same charge
partitions in the same order, the same tensors bit for bit, the same ``valid`` flags and meta records -- without a
Python object per spectrum or per peak and without the reference package: the text is uploaded in chunks, split
into lines, classified and converted by the kernels of ``csrc/sptxt.hip`` (``asl_sptxt_measure`` /
``asl_sptxt_fill``, then ``asl_mgf_sort_charged``), and the raw pack goes to the existing ``process_spectra`` where
it lies. The host's part: the few numerals the device defers (Python's ``float``), the peptide strings (``proforma``,
from byte ranges the device returns), the checks a whole record must pass and the meta records.

The dialect is stated in ``include/annsolo_mi.h`` and restated in ``tests/sptxt_ref.py``. pyteomics and
spectrum_utils are not dependencies: the statement is unpinned, like the MGF reader's.
"""
import ctypes as C
import io
import logging
import math
import os
import re
import time
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .packed import PackedSpectra

MAX_PEAKS = _lib.MGF_MAX_PEAKS      # peak lines of one record (ASL_MGF_MAX_PEAKS)
MAX_CHUNK = (1 << 31) - 1           # bytes of one chunk: the ABI's limit
PROCESS_ROWS = 1 << 15              # spectra per ``process_spectra`` call
READER_VERSION = 1                  # in the packed store's key (``library_store.store_hash``)

# counts[] of asl_sptxt_measure
_N_LINES, _N_RECORDS, _N_PEAKS, _N_DEFERRED, _CONSUMED, _CONSUMED_LINES, _ERR_KIND, _ERR_LINE, _OPEN = range(9)
_DEST_MZ, _DEST_INTENSITY, _DEST_PRECURSOR, _DEST_NONE = range(4)
_INFO = 8                           # ASL_SPTXT_INFO
_ERR_TEXT = {1: 'a second Name: in the line', 2: 'a second Num Peaks line in the record',
             3: 'a Num Peaks line that is not "Num Peaks: <digits>"', 4: 'a peak line with fewer than three fields',
             5: 'a PrecursorMZ line that is not "PrecursorMZ: <digits[.digits]>"',
             6: 'a PrecursorMZ: or Num Peaks: key inside a metadata line'}
_PEPTIDE = re.compile(r'[A-Z]+')
_INDEX = re.compile(r'-?[0-9]+')


def is_sptxt(filename) -> bool:
    return os.fspath(filename).lower().endswith('.sptxt')


def proforma(peptide: str, mods: Optional[str]) -> str:
    """The ProForma string of a Name-line peptide and the record's ``Mods=`` value (the text behind the key up to
    the first blank, ``count/index,residue,name/...``; ``None``: no ``Mods=``): ``[name]`` goes behind residue
    ``index``, so index -1 lands in front of the first letter. The count and the residue letters are not read.
    ``ValueError`` for a peptide that is not upper-case letters only, a field that is not ``index,residue,name``,
    an index outside -1 .. len - 1, or indices that descend (the reference's running shift then misplaces them)."""
    if not _PEPTIDE.fullmatch(peptide):
        raise ValueError(f'peptide {peptide!r} is not upper-case letters only')
    if mods is None:
        return peptide
    out = list(peptide)
    before = -1
    for shift, field in enumerate(mods.split('/')[1:]):
        parts = field.split(',')
        if len(parts) != 3 or not _INDEX.fullmatch(parts[0]):
            raise ValueError(f'modification {field!r} is not index,residue,name')
        idx = int(parts[0])
        if not -1 <= idx < len(peptide) or idx < before:
            raise ValueError(f'modification {field!r}: index outside -1 .. {len(peptide) - 1}, or descending')
        before = idx
        out.insert(idx + shift + 1, '[' + parts[2] + ']')
    return ''.join(out)


def _float(token: bytes):
    """(value, None) or (None, reason)."""
    try:
        v = float(token)
    except ValueError:
        return None, f'{token!r} is not a number'
    if not math.isfinite(v):
        return None, f'non-finite {token!r}'
    return v, None


class _Reader:
    def __init__(self, device, stats: Optional[dict]):
        self.device = torch.device(device)
        self.timed = stats is not None      # only then are the parts synchronised for their timers
        self.stats = stats if stats is not None else {}
        self.stats.update(chunks=0, n_lines=0, n_records=0, n_peaks=0, n_deferred=0, n_sorted=0, grown=0,
                          read_s=0.0, parse_s=0.0, process_s=0.0)
        self.line0 = 0                      # lines of the file before the chunk
        self.rec0 = 0                       # records of the file before the chunk
        self.sink = None                    # called with (raw pack on the device, columns) per chunk

    def _sync(self) -> None:
        if self.timed and self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    @staticmethod
    def _raise_first(errors) -> None:
        if errors:
            raise ValueError('sptxt: ' + min(errors, key=lambda e: (e[0], e[1]))[2])

    def chunk(self, buf: bytearray, text: torch.Tensor, counts: np.ndarray, end_line: int) -> None:
        """Fill, patch, check and sort the closed records of the measured chunk ``buf`` (``text`` on the device),
        then hand them to the sink. ``end_line``: the lines of the chunk this call consumes."""
        dev, n = self.device, len(buf)
        ns, npk, nd = int(counts[_N_RECORDS]), int(counts[_N_PEAKS]), int(counts[_N_DEFERRED])
        errors = []                         # (line or surrogate, 0 line-level | 1 record-level, message)
        if counts[_ERR_KIND]:
            ln = int(counts[_ERR_LINE])
            errors.append((ln, 0, f'line {self.line0 + ln + 1}: {_ERR_TEXT[int(counts[_ERR_KIND])]}'))
        if ns == 0:
            self._raise_first(errors)
            return
        t0 = time.perf_counter()
        offsets = torch.empty(ns + 1, dtype=torch.int32, device=dev)
        mz = torch.empty(npk, dtype=torch.float32, device=dev)
        it = torch.empty(npk, dtype=torch.float32, device=dev)
        chg = torch.empty(npk, dtype=torch.uint8, device=dev)
        pmz = torch.empty(ns, dtype=torch.float64, device=dev)
        info = torch.empty((ns, _INFO), dtype=torch.int32, device=dev)
        rec = torch.empty((nd, 5), dtype=torch.int32, device=dev)
        opt = lambda a: _lib.ptr(a) if a.numel() else None
        _lib.check(_lib.lib().asl_sptxt_fill(_lib.ptr(text), n, _lib.ptr(offsets), opt(mz), opt(it), opt(chg),
                                             _lib.ptr(pmz), _lib.ptr(info), opt(rec)))
        pmz_h, info_h, off_h = pmz.cpu().numpy(), info.cpu().numpy(), offsets.cpu().numpy()
        first_h = info_h[:, 7]
        # record-level errors stand at the line behind their record
        behind = np.append(first_h[1:], end_line).astype(np.int64)
        bad_pmz = {}                        # record -> why its deferred precursor numeral was refused
        if nd:
            slots = {_DEST_MZ: ([], []), _DEST_INTENSITY: ([], [])}      # kind -> (peak slots, values)
            for o, l, kind, idx, ln in rec.cpu().numpy().tolist():
                if kind == _DEST_NONE:
                    continue
                v, why = _float(bytes(buf[o:o + l]))
                if kind == _DEST_PRECURSOR:
                    if why:
                        bad_pmz[idx] = why
                    else:
                        pmz_h[idx] = v
                elif why:
                    what = 'm/z' if kind == _DEST_MZ else 'intensity'
                    errors.append((ln, 0, f'line {self.line0 + ln + 1}: {what} {why}'))
                else:
                    slots[kind][0].append(idx)
                    slots[kind][1].append(v)
            for kind, column in ((_DEST_MZ, mz), (_DEST_INTENSITY, it)):
                if slots[kind][0]:
                    with np.errstate(over='ignore'):        # (a finite double beyond float32 is inf there)
                        v32 = np.asarray(slots[kind][1], np.float64).astype(np.float32)
                    column[torch.as_tensor(slots[kind][0], dtype=torch.int64, device=dev)] = \
                        torch.as_tensor(v32, device=dev)
        # what a whole record must satisfy, in the order the restatement checks it; the first failure ends the look
        peptides: List[Optional[str]] = [None] * ns
        view = memoryview(buf)
        cut = lambda o, l: bytes(view[o:o + l]).decode('utf-8', 'replace')
        n_peaks = np.diff(off_h)
        for s, (z, status, _, na, nl, ma, ml, _) in enumerate(info_h.tolist()):
            why = None
            if nl < 0:
                why = 'the Name line has no "/"'
            elif z < 0:
                why = 'precursor charge is not digits in 1 .. 255'
            else:
                try:
                    peptides[s] = proforma(cut(na, nl), cut(ma + 5, ml - 5) if ml >= 0 else None)
                except ValueError as e:
                    why = str(e)
            if why is None:
                if status == 1:
                    why = 'neither a PrecursorMZ line nor Parent='
                elif status == 2:
                    why = 'the Parent= numeral is not digits[.digits]'
                elif s in bad_pmz:
                    why = f'precursor m/z {bad_pmz[s]}'
                elif n_peaks[s] == 0:
                    why = 'no peak lines'
            if why is not None:
                errors.append((int(behind[s]), 1, f'record {self.rec0 + s + 1}: {why}'))
                break
        del view
        self._raise_first(errors)
        n_sorted = C.c_int64(0)
        _lib.check(_lib.lib().asl_mgf_sort_charged(_lib.ptr(offsets), opt(mz), opt(it), opt(chg), ns, npk,
                                                   C.byref(n_sorted)))
        pz_h = np.ascontiguousarray(info_h[:, 0], np.int32)
        ids = [str(self.rec0 + s + 1) for s in range(ns)]
        raw = PackedSpectra(offsets, mz, it, chg, torch.as_tensor(pmz_h, device=dev),
                            torch.as_tensor(pz_h, device=dev), identifiers=ids)
        self._sync()
        t1 = time.perf_counter()
        self.sink(raw, dict(identifier=ids, peptide=peptides, precursor_mz=pmz_h, precursor_charge=pz_h,
                            is_decoy=info_h[:, 2].astype(bool)))
        self._sync()
        st = self.stats
        st['parse_s'] += t1 - t0
        st['process_s'] += time.perf_counter() - t1
        st['n_records'] += ns
        st['n_peaks'] += npk
        st['n_deferred'] += nd
        st['n_sorted'] += int(n_sorted.value)

    # ------------------------------------------------------------------ the file
    def read(self, f, chunk_bytes: int) -> None:
        size = max(int(chunk_bytes), 1)
        if size > MAX_CHUNK:
            raise ValueError(f'chunk_bytes = {chunk_bytes}: at most {MAX_CHUNK}')
        buf, eof = bytearray(), False
        while True:
            t0 = time.perf_counter()
            want = size - len(buf)
            if want > 0 and not eof:
                more = f.read(want)
                eof = len(more) < want
                buf += more
            n, last = len(buf), eof
            if n == 0:
                break
            t1 = time.perf_counter()
            text = torch.frombuffer(buf, dtype=torch.uint8).to(self.device)
            counts = np.zeros(16, np.int64)
            _lib.check(_lib.lib().asl_sptxt_measure(_lib.ptr(text), n, int(last),      # (returns synchronised)
                                                    counts.ctypes.data_as(_lib.c_i64p)))
            self.stats['read_s'] += t1 - t0
            self.stats['parse_s'] += time.perf_counter() - t1
            n_lines = int(counts[_N_LINES])
            if last or counts[_OPEN]:
                consumed, end_line = int(counts[_CONSUMED]), int(counts[_CONSUMED_LINES])
            elif buf.endswith(b'\n'):       # no record yet: the preamble's whole lines
                consumed, end_line = n, n_lines
            else:                           # a cut last line: it may be the start of a Name line
                consumed, end_line = buf.rfind(b'\n') + 1, n_lines - 1
            if consumed == 0 and not last:  # one record (or line) does not fit: a larger chunk
                if size >= MAX_CHUNK:
                    err = _lib.AnnSoloMiError(f'sptxt: record {self.rec0 + 1} does not fit a chunk of '
                                              f'{MAX_CHUNK} bytes')
                    err.code = _lib.ERR_CAPACITY
                    raise err
                size = min(2 * size, MAX_CHUNK)
                self.stats['grown'] += 1
                del text
                continue
            self.chunk(buf, text, counts, end_line)
            self.stats['chunks'] += 1
            self.stats['n_lines'] += end_line
            self.line0 += end_line
            self.rec0 += int(counts[_N_RECORDS])
            del text
            del buf[:consumed]
            if last:
                break


def _read(reader: _Reader, source, chunk_bytes: int) -> None:
    if isinstance(source, (str, os.PathLike)):
        with open(source, 'rb') as f:
            reader.read(f, chunk_bytes)
    else:
        reader.read(io.BytesIO(bytes(source)), chunk_bytes)


def read_sptxt_raw(source, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The parse alone: ``(packs, columns)`` -- per chunk the records' raw ``PackedSpectra`` on ``device`` (what
    ``library_store.pack_raw`` makes of the restatement's objects: float32 peaks with their fragment charges, stably
    sorted by m/z where they descend) and the per-record columns ``identifier`` (the ordinal in the file as a
    string), ``peptide`` (ProForma), ``precursor_mz`` (float64), ``precursor_charge`` and ``is_decoy``, each over all
    chunks. ``source``: a path, or the file's bytes. The file is read in chunks of ``chunk_bytes``; the bytes from the
    last Name line on are carried into the next chunk, and a chunk that holds no whole record is doubled, up to
    ``MAX_CHUNK``. ``stats`` receives what the reader counted (``chunks``, ``grown``, ``n_lines``, ``n_records``,
    ``n_peaks``, ``n_deferred`` -- tokens left to Python's ``float()`` --, ``n_sorted``, and the seconds ``read_s``,
    ``parse_s``, ``process_s``). Deviations of the dialect raise ``ValueError`` naming the 1-based line or record; a
    record of more than ``MAX_PEAKS`` peak lines, or a line of more than ``_lib.MGF_MAX_LINE`` bytes, raises
    ``AnnSoloMiError`` with ``code == ERR_CAPACITY``."""
    reader = _Reader(device, stats)
    packs, cols = [], []
    reader.sink = lambda raw, c: (packs.append(raw), cols.append(c))
    _read(reader, source, chunk_bytes)
    return packs, _join_columns(cols)


def _join_columns(cols: List[dict]) -> dict:
    return dict(identifier=[i for c in cols for i in c['identifier']],
                peptide=[p for c in cols for p in c['peptide']],
                precursor_mz=np.concatenate([c['precursor_mz'] for c in cols]) if cols else np.zeros(0, np.float64),
                precursor_charge=(np.concatenate([c['precursor_charge'] for c in cols]) if cols
                                  else np.zeros(0, np.int32)),
                is_decoy=np.concatenate([c['is_decoy'] for c in cols]) if cols else np.zeros(0, bool))


class SptxtLibrary:
    """The library of a ``.sptxt`` file behind the reference reader's surface (``spec_info``, ``is_recreated``,
    ``get_version()``, ``close()``, ``_filename``) with its packed ``store``. ``read_all_spectra()`` is not
    offered: nothing here holds spectrum objects."""

    def __init__(self, filename, store, is_recreated: bool):
        self._filename = filename
        self.store = store
        self.is_recreated = is_recreated
        pmz, ids = store.spectra.precursor_mz.numpy(), store.spectra.identifiers
        self.spec_info = {'charge': {z: {'id': np.asarray(ids[a:b]), 'precursor_mz': pmz[a:b].astype(np.float32)}
                                     for z, (a, b) in store.ranges.items()}}

    def get_version(self) -> str:
        return 'null'

    def close(self) -> None:
        pass

    def read_all_spectra(self):
        raise NotImplementedError('the device library reader keeps no spectrum objects: use .store')


def build_store(source, config=None, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None,
                process_rows: int = PROCESS_ROWS):
    """The ``LibraryStore`` of the file: charges in order of first appearance, rows in file order inside a charge
    (the reference's ``spec_info`` order), every spectrum preprocessed with ``is_library=True``. With
    ``config.device_decoys`` every record gives two rows, its shuffle-and-reposition decoy and then itself with the
    decoy generator's fragment charges, as ``library_store.DecoyReader`` lists them."""
    from .config import Config
    from .library_store import LibraryStore, concat_packs
    from .spectrum import process_spectra
    cfg = Config.from_reference(config)
    reader = _Reader(device, stats)
    outs, valids, cols = [], [], []

    def sink(raw: PackedSpectra, c: dict) -> None:
        if cfg.device_decoys:
            from . import decoy_generator as dg
            decoy, names, ann = dg.shuffle_and_reposition_batch(raw, c['peptide'], cfg.fragment_mz_tolerance,
                                                                cfg.decoy_tolerance_unit, cfg.seed, reader.device)
            target = PackedSpectra(raw.offsets, raw.mz, raw.intensity, ann['z'], raw.precursor_mz,
                                   raw.precursor_charge, identifiers=raw.identifiers)
            both = concat_packs([decoy, target])
            order = np.arange(2 * raw.n).reshape(2, raw.n).T.reshape(-1)      # decoy row, target row
            raw = both.select(torch.as_tensor(order))
            two = lambda a: np.repeat(np.asarray(a), 2)
            ids, pep = np.repeat(np.asarray(c['identifier'], object), 2), np.repeat(np.asarray(c['peptide'], object), 2)
            ids[0::2] = ['DECOY_' + i for i in c['identifier']]
            pep[0::2] = names
            dec = two(c['is_decoy'])
            dec[0::2] = True
            c = dict(identifier=ids.tolist(), peptide=pep.tolist(), precursor_mz=two(c['precursor_mz']),
                     precursor_charge=two(c['precursor_charge']), is_decoy=dec)
        for a in range(0, raw.n, process_rows):
            part = raw if raw.n <= process_rows else raw.select(torch.arange(a, min(a + process_rows, raw.n)))
            out, valid = process_spectra(part, True, cfg, reader.device)
            outs.append(out.to('cpu'))
            valids.append(valid.cpu().numpy().astype(bool))
        cols.append(c)

    reader.sink = sink
    _read(reader, source, chunk_bytes)
    c = _join_columns(cols)
    n = len(c['identifier'])
    pz = c['precursor_charge']
    charges = list(dict.fromkeys(pz.tolist()))
    rank = {z: r for r, z in enumerate(charges)}
    order = np.argsort(np.asarray([rank[z] for z in pz.tolist()], np.int64), kind='stable')
    if n:
        flat = concat_packs(outs).select(torch.as_tensor(order))
        valid = np.concatenate(valids)[order]
    else:
        z = lambda dt: torch.zeros(0, dtype=dt)
        flat = PackedSpectra(torch.zeros(1, dtype=torch.int32), z(torch.float32), z(torch.float32), z(torch.uint8),
                             z(torch.float64), z(torch.int32))
        valid = np.zeros(0, bool)
    ids = [c['identifier'][i] for i in order]
    flat = PackedSpectra(flat.offsets, flat.mz, flat.intensity, flat.charge, flat.precursor_mz,
                         flat.precursor_charge, identifiers=ids)
    ranges, meta, base = {}, {}, 0
    for z in charges:
        k = int((pz == z).sum())
        ranges[int(z)] = (base, base + k)
        meta[int(z)] = [dict(identifier=c['identifier'][i], peptide=c['peptide'][i],
                             precursor_mz=float(c['precursor_mz'][i]), is_decoy=bool(c['is_decoy'][i]))
                        for i in order[base:base + k]]
        base += k
    return LibraryStore(flat, valid, ranges, meta)


def file_stamp(filename) -> dict:
    st = os.stat(filename)
    return {'size': int(st.st_size), 'mtime_ns': int(st.st_mtime_ns)}


def read_library(filename, config=None, device='cuda', path: Optional[str] = None, key: str = '',
                 chunk_bytes: int = 256 << 20, stats: Optional[dict] = None) -> SptxtLibrary:
    """The library of ``filename``: its packed store is loaded from ``path`` when that file was written under
    ``key`` for a library file of the same size and modification time, else built by ``build_store`` (and written
    when ``path`` is given), and then ``is_recreated`` is set, so that the caller rebuilds its indexes too. Neither a
    ``.spcfg`` nor an ``.hdf5`` is written."""
    from . import library_store as ls
    filename = os.fspath(filename)
    stamp = file_stamp(filename)
    if path and os.path.isfile(path):
        try:
            st = ls.load_library_store(path, key)
            if st.source == stamp:
                return SptxtLibrary(filename, st, False)
            logging.warning('Packed library store %s was built from another %s: rebuilding', path, filename)
        except (ValueError, KeyError, OSError) as e:
            logging.warning('Packed library store %s unusable (%s): rebuilding', path, e)
    st = build_store(filename, config, device, chunk_bytes, stats)
    st.source = stamp
    if path:
        ls.save_library_store(st, path, key)
    return SptxtLibrary(filename, st, True)
