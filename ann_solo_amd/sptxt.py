"""SpectraST ``.sptxt`` libraries read on the device (``Config.device_library``; DESIGN.md 3 "Library files").

``read_library(filename, config, device)`` returns a reader object that holds the ``LibraryStore``
``library_store.build_library_store`` makes of the same file read record by record in Python -- the same charge
partitions in the same order, the same tensors bit for bit, the same ``valid`` flags and meta records -- without a
Python object per spectrum or per peak and without the reference package: the text is uploaded in chunks, split
into lines, classified and converted by the kernels of ``csrc/sptxt.hip`` (``asl_sptxt_measure`` /
``asl_sptxt_fill``, then ``asl_mgf_sort_charged``), and the raw pack goes to the existing ``process_spectra`` where
it lies. The host's part: the few numerals the device defers (Python's ``float``), the peptide strings (``proforma``,
from byte ranges the device returns), the checks a whole record must pass and the meta records. The chunk loop and
what else is not about the dialect is ``text_reader.ChunkedReader``, shared with ``mgf.py``.

The dialect is stated in ``include/annsolo_mi.h`` and restated in ``tests/sptxt_ref.py``. pyteomics and
spectrum_utils are not dependencies: the statement is unpinned, like the MGF reader's.
"""
import ctypes as C
import logging
import os
import re
import time
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .packed import PackedSpectra
from .text_reader import MAX_CHUNK, N_DEFERRED, N_PEAKS, N_RECORDS, ChunkedReader, opt

MAX_PEAKS = _lib.MGF_MAX_PEAKS      # peak lines of one record (ASL_MGF_MAX_PEAKS)
PROCESS_ROWS = 1 << 15              # spectra per ``process_spectra`` call
READER_VERSION = 1                  # in the packed store's key (``library_store.store_hash``)

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


class _Reader(ChunkedReader):
    PREFIX, RECORD, COUNT_KEY, ERR_TEXT = 'sptxt: ', 'record', 'n_records', _ERR_TEXT

    def __init__(self, device, stats: Optional[dict]):
        super().__init__(device, stats)
        self.sink = None                    # called with (raw pack on the device, columns) per chunk

    def measure(self, text: torch.Tensor, n: int, last: bool) -> np.ndarray:
        counts = np.zeros(16, np.int64)
        _lib.check(_lib.lib().asl_sptxt_measure(_lib.ptr(text), n, int(last), counts.ctypes.data_as(_lib.c_i64p)))
        return counts

    def chunk(self, buf: bytearray, text: torch.Tensor, counts: np.ndarray, end_line: int) -> None:
        """Fill, patch, check and sort the closed records of the measured chunk ``buf`` (``text`` on the device),
        then hand them to the sink. ``end_line``: the lines of the chunk this call consumes."""
        dev, n = self.device, len(buf)
        ns, npk, nd = int(counts[N_RECORDS]), int(counts[N_PEAKS]), int(counts[N_DEFERRED])
        errors = self.structural_errors(counts)
        if ns == 0:
            self._raise_first(errors)
            return
        t0 = time.perf_counter()
        offsets, mz, it, chg, pmz, rec = self.columns(ns, npk, nd)
        info = torch.empty((ns, _INFO), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().asl_sptxt_fill(_lib.ptr(text), n, _lib.ptr(offsets), opt(mz), opt(it), opt(chg),
                                             _lib.ptr(pmz), _lib.ptr(info), opt(rec)))
        pmz_h, info_h, off_h = pmz.cpu().numpy(), info.cpu().numpy(), offsets.cpu().numpy()
        behind = self.behind(info_h[:, 7], end_line)
        bad_pmz = {}                        # record -> why its deferred precursor numeral was refused

        def precursor_numeral(kind, idx, v, why):       # (_DEST_PRECURSOR: a record's only deferred numeral)
            if why:
                bad_pmz[idx] = why
            else:
                pmz_h[idx] = v
        if nd:
            self.patch_deferred(buf, rec, mz, it, _DEST_NONE, errors, precursor_numeral)
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
        self.account(t0, t1, ns, npk, nd, int(n_sorted.value))


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
    reader.read_source(source, chunk_bytes)
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
    reader.read_source(source, chunk_bytes)
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
