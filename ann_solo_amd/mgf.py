"""MGF query files read on the device (``Config.device_mgf``; DESIGN.md 3 "Query files").

``read_mgf_packed(source, config, device)`` returns what ``library_store.pack_queries`` returns for the
spectra of an MGF file -- the same charges in the same order, the same tensors bit for bit, the same meta
records -- without a Python object per spectrum or per peak: the text is uploaded in chunks, split into lines,
classified and converted by the kernels of ``csrc/mgf.hip`` (``asl_mgf_measure`` / ``asl_mgf_fill`` /
``asl_mgf_sort``), and the raw pack goes to the existing ``process_spectra`` where it lies. The host's part: the
header (a few lines before the first ``BEGIN IONS``), the few numerals the device defers (Python's ``float``),
the identifiers (UTF-8 slices of the chunk) and the meta records. The chunk loop and what else is not about the
dialect is ``text_reader.ChunkedReader``, shared with ``sptxt.py``, and what follows the parse
``text_reader.QueryReader``, shared with ``mzml.py``; the sort is ``csrc/peak_sort.hip``.

The dialect is stated in ``include/annsolo_mi.h`` and restated in ``tests/mgf_ref.py``. pyteomics is not a
dependency: the statement is unpinned, like FAISS and spectrum_utils elsewhere in this package.
"""
import ctypes as C
import logging
import re
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .packed import PackedSpectra
from .text_reader import MAX_CHUNK, N_DEFERRED, N_PEAKS, N_RECORDS, OPEN, QueryReader, _float, opt

SCAN_TILE = _lib.MGF_TILE           # lines per workgroup of the reader's scans (ASL_MGF_TILE)
MAX_PEAKS = _lib.MGF_MAX_PEAKS      # peak lines of one spectrum (ASL_MGF_MAX_PEAKS)

_DEST_MZ, _DEST_INTENSITY, _DEST_PEPMASS, _DEST_RT, _DEST_NONE = range(5)
_ERR_TEXT = {1: 'BEGIN IONS inside a block', 2: 'a peak line with one token'}
_COMMENT = (b'#', b';', b'!', b'/')
_CHARGE_SPLIT = re.compile(rb'(?:,\s*)|(?:\s*and\s*)')
_CHARGE = re.compile(rb'([+-]?)([0-9]+)|([0-9]+)([+-])')


def _header_charge(value: bytes) -> int:
    """The first element of a charge list, as the kernel reads it: 1 .. 255, else -1."""
    m = _CHARGE.fullmatch(_CHARGE_SPLIT.split(value)[0].strip())
    if m is None:
        return -1
    sign, digits = (m.group(1), m.group(2)) if m.group(2) is not None else (m.group(4), m.group(3))
    z = int(digits)
    return z if sign != b'-' and 1 <= z <= 255 else -1


class _Header:
    """The lines with ``=`` before the first ``BEGIN IONS``: the defaults of every block."""

    def __init__(self):
        self.params: Dict[bytes, bytes] = {}
        self.done = False

    def feed(self, data, end: int) -> None:
        pos = 0
        while pos < end and not self.done:
            nl = data.find(b'\n', pos, end)
            stop = end if nl < 0 else nl
            line = bytes(data[pos:stop]).strip()
            pos = stop + 1
            if line == b'BEGIN IONS':
                self.done = True
            elif b'=' in line and line[:1] not in _COMMENT:
                k, v = line.split(b'=', 1)
                self.params[k.lower()] = v.strip()


class _Reader(QueryReader):
    PREFIX, RECORD, COUNT_KEY, ERR_TEXT = 'MGF: ', 'a block of spectrum', 'n_spectra', _ERR_TEXT

    def __init__(self, config, device, stats: Optional[dict], keep_raw: bool = False):
        super().__init__(config, device, stats, keep_raw)
        self.header = _Header()

    # ------------------------------------------------------------------ one chunk
    def measure(self, text: torch.Tensor, n: int, last: bool) -> np.ndarray:
        counts = np.zeros(16, np.int64)
        _lib.check(_lib.lib().asl_mgf_measure(_lib.ptr(text), n, int(last), counts.ctypes.data_as(_lib.c_i64p)))
        return counts

    def before_chunk(self, buf: bytearray, consumed: int, counts: np.ndarray, last: bool) -> None:
        if last and counts[OPEN]:
            logging.warning('MGF: the last block is not closed at the end of the file: dropped')
        self.header.feed(buf, consumed)

    def chunk(self, buf: bytearray, text: torch.Tensor, counts: np.ndarray, end_line: int) -> None:
        """Fill, patch, sort and preprocess the closed blocks of the measured chunk ``buf`` (``text`` on the
        device). ``end_line``: the lines of the chunk this call consumes."""
        dev, n = self.device, len(buf)
        ns, npk, nd = int(counts[N_RECORDS]), int(counts[N_PEAKS]), int(counts[N_DEFERRED])
        errors = self.structural_errors(counts)
        if ns == 0 and nd == 0:
            self._raise_first(errors)
            return
        t0 = time.perf_counter()
        offsets, mz, it, chg, pmz, rec = self.columns(ns, npk, nd)
        pz = torch.empty(ns, dtype=torch.int32, device=dev)
        rt = torch.empty(ns, dtype=torch.float64, device=dev)
        ident = torch.empty((ns, 2), dtype=torch.int32, device=dev)
        first = torch.empty(ns, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().asl_mgf_fill(_lib.ptr(text), n, _lib.ptr(offsets), opt(mz), opt(it), opt(chg),
                                           opt(pmz), opt(pz), opt(rt), opt(ident), opt(first), opt(rec)))
        pmz_h, pz_h, rt_h = pmz.cpu().numpy(), pz.cpu().numpy(), rt.cpu().numpy()
        ident_h, first_h = ident.cpu().numpy(), first.cpu().numpy()
        behind = self.behind(first_h, end_line)

        def block_numeral(kind, idx, v, why):           # a PEPMASS or RTINSECONDS numeral the device deferred
            what = 'pepmass' if kind == _DEST_PEPMASS else 'rtinseconds'
            if why:
                errors.append((int(behind[idx]), 1, f'spectrum {self.rec0 + idx + 1}: {what} {why}'))
                v = 0.0
            (pmz_h if kind == _DEST_PEPMASS else rt_h)[idx] = v
        if nd:
            self.patch_deferred(buf, rec, mz, it, _DEST_NONE, errors, block_numeral)
        if ns == 0:                         # nothing but an unclosed last block
            self._raise_first(errors)
            return
        # the header's defaults and the per-block deviations
        hp = self.header.params
        ids = self._identifiers(buf, ident_h, hp, errors, behind)
        missing = np.isnan(pmz_h)
        if missing.any():
            tok = hp.get(b'pepmass', None)
            if tok is None:
                s = int(np.argmax(missing))
                errors.append((int(behind[s]), 1, f'spectrum {self.rec0 + s + 1}: no PEPMASS'))
            else:
                first_tok = tok.split()
                v, why = _float(first_tok[0] if first_tok else b'')
                if why:
                    s = int(np.argmax(missing))
                    errors.append((int(behind[s]), 1, f'spectrum {self.rec0 + s + 1}: pepmass {why}'))
                    v = 0.0
                pmz_h[missing] = v
        if b'charge' in hp and (pz_h == 0).any():
            pz_h[pz_h == 0] = _header_charge(hp[b'charge'])
        if (pz_h < 0).any():
            s = int(np.argmax(pz_h < 0))
            errors.append((int(behind[s]), 1, f'spectrum {self.rec0 + s + 1}: charge outside 1 .. 255'))
        rt_none = np.isnan(rt_h)
        if b'rtinseconds' in hp and rt_none.any():
            v, why = _float(hp[b'rtinseconds'])
            if why:
                s = int(np.argmax(rt_none))
                errors.append((int(behind[s]), 1, f'spectrum {self.rec0 + s + 1}: rtinseconds {why}'))
            else:
                rt_h[rt_none] = v
                rt_none = np.zeros(ns, bool)
        self._raise_first(errors)
        n_sorted = C.c_int64(0)
        _lib.check(_lib.lib().asl_mgf_sort(_lib.ptr(offsets), opt(mz), opt(it), ns, npk, C.byref(n_sorted)))
        raw = PackedSpectra(offsets, mz, it, chg, torch.as_tensor(pmz_h, device=dev),
                            torch.as_tensor(pz_h, device=dev))
        self._sync()
        t1 = time.perf_counter()
        self.take(raw, pz_h, pmz_h, rt_h, rt_none, ids, self.rec0 + 1 + np.arange(ns))
        self.account(t0, t1, ns, npk, nd, int(n_sorted.value))

    def _identifiers(self, buf, ident_h, hp, errors, behind) -> List[Optional[str]]:
        """title, else scan, of the block over the header's: the identifiers as str."""
        h_title, h_scan = hp.get(b'title'), hp.get(b'scan')
        ids: List[Optional[str]] = []
        for s, (o, l) in enumerate(ident_h.tolist()):
            if l >= 0 and h_title is not None:
                # (the header's title goes before the block's scan: which of the two did the block give?)
                key = bytes(buf[buf.rfind(b'\n', 0, o) + 1:o]).lstrip().split(b'=', 1)[0].lower()
                if key != b'title':
                    l = -1
            if l >= 0:
                ids.append(bytes(buf[o:o + l]).decode('utf-8'))
            elif h_title is not None or h_scan is not None:
                ids.append((h_title if h_title is not None else h_scan).decode('utf-8'))
            else:
                errors.append((int(behind[s]), 1, f'spectrum {self.rec0 + s + 1}: neither TITLE nor SCAN'))
                ids.append(None)
        return ids


def read_mgf_raw(source, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The parse alone: ``(raw, retention_time, identifiers)`` -- the file's spectra as one raw
    ``PackedSpectra`` on ``device`` (what ``library_store.pack_raw`` makes of the reader's objects: float32
    peaks in file order, stably sorted by m/z where they descend; precursor charge 0 = unknown), the retention
    times (float64 numpy, NaN = none) and the identifiers. Arguments and errors as ``read_mgf_packed``."""
    reader = _Reader(None, device, stats, keep_raw=True)
    reader.read_source(source, chunk_bytes)
    return reader.raw_result()[:3]


def read_mgf_packed(source, config=None, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The spectra of an MGF file as ``library_store.pack_queries`` returns them: ``({charge: PackedSpectra},
    {charge: [meta]})``, preprocessed, charges in order of first appearance, queries of unknown charge entered
    at 2 and 3, invalid spectra dropped. ``source``: a path, or the file's bytes. The file is read in chunks of
    ``chunk_bytes``; the bytes behind the last closed block are carried into the next chunk, and a chunk that
    holds no whole block is doubled, up to ``MAX_CHUNK``. ``stats``: a dict that receives what the reader
    counted (``chunks``, ``grown``, ``n_lines``, ``n_spectra``, ``n_peaks``, ``n_deferred`` -- tokens the device
    left to Python's ``float()`` --, ``n_sorted`` -- spectra the device had to sort --, and the seconds spent
    reading the file (``read_s``), parsing (``parse_s``: upload, kernels, deferred numerals, identifiers and
    columns) and preprocessing with the meta records (``process_s``)). Deviations of the dialect raise ``ValueError`` naming the 1-based line or spectrum; a
    spectrum of more than ``MAX_PEAKS`` peak lines, or a line of more than ``_lib.MGF_MAX_LINE`` bytes, raises
    ``AnnSoloMiError`` with ``code == ERR_CAPACITY`` (before the ``ValueError``s of the same chunk). An unclosed
    last block is dropped with a warning; a deviation on one of its lines is reported like any other."""
    reader = _Reader(config, device, stats)
    reader.read_source(source, chunk_bytes)
    return reader.result()
