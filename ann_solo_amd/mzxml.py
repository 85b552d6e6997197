"""mzXML query files read on the device (``Config.device_mzxml``; DESIGN.md 3 "Query files").

``read_mzxml_packed(source, config, device)`` returns what ``library_store.pack_queries`` returns for the MS2 scans
the reference's ``read_mzxml`` yields from an mzXML file -- the same charges in the same order, the same tensors bit
for bit, the same meta records -- without pyteomics, lxml, or a Python object per scan: the text is uploaded in
chunks, split into tags, classified, and each MS2 scan's one base64 / zlib stream of interleaved big-endian pairs
decoded by the kernels of ``csrc/mzxml.hip`` (``asl_mzxml_measure`` / ``asl_mzxml_fill``, then ``asl_mgf_sort``), and
the raw pack goes to the existing ``process_spectra`` where it lies. The host's part: the identifiers (Python's own
``int`` over ``num``), the few numerals and the durations the device defers (``duration_minutes``), the error codes
turned into ``ValueError`` and the meta records. The chunk loop is ``text_reader.ChunkedReader``, what follows the
parse ``text_reader.QueryReader``, both shared with ``mgf.py`` and ``mzml.py``. A chunk's record is a scan's head --
its tags up to the next ``<scan`` or ``</scan>`` -- so a chunk may end inside a scan whose children are still to
come; the ordinal of the next scan and the nesting depth are all that crosses a cut.

The dialect is stated in ``include/annsolo_mi.h`` and restated in ``tests/mzxml_ref.py``. pyteomics is not a
dependency: the statement is unpinned, like the mzML reader's.
"""
import ctypes as C
import logging
import re
import time
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .mzml import unescape
from .packed import PackedSpectra
from .text_reader import ERR_KIND, ERR_LINE, N_PEAKS, N_RECORDS, OPEN, QueryReader, _float, opt

SCAN_TILE = _lib.MGF_TILE               # tags per workgroup of the reader's scans (ASL_MGF_TILE)
MAX_PEAKS = _lib.MGF_MAX_PEAKS          # peaksCount of one scan (ASL_MGF_MAX_PEAKS)
MAX_TAG = _lib.MZML_MAX_TAG             # bytes of one tag (ASL_MZML_MAX_TAG)

N_ELEMENTS, ERR_ELEMENT, DEPTH_ALL, DEPTH_CONSUMED = 9, 10, 11, 12     # counts[] behind the shared ones
_ERR_TEXT = {1: 'a <precursorMz> or <peaks> outside any scan', 2: 'a comment or CDATA section after the first <scan',
             3: 'a tag that does not end', 4: 'an msLevel that is not a number'}
# errors[] of asl_mzxml_fill (ASL_MZXML_E_*)
_E_FILE = 0x7f
_E_TEXT = [(0x1, 'peaksCount is missing or not a number'), (0x2, 'no <peaks>'), (0x4, 'more than one <peaks>'),
           (0x8, 'a missing or unsupported precision (32 or 64)'), (0x10, 'a byteOrder other than network'),
           (0x20, 'a contentType or pairOrder other than m/z-int'),
           (0x40, 'an unsupported compressionType (none or zlib)'),
           (0x100, 'no retentionTime'), (0x200, 'no <precursorMz>'),
           (0x400, 'a precursorCharge that is not a number in 1 .. 255')]
_F_ZLIB, _F_F64, _F_NESTED = 1, 2, 4    # flags[] (ASL_MZXML_F_*)

_NUM = r'(\d+\.?\d*)'
_DURATION = re.compile(rf'P(?:\d+\.?\d*Y)?(?:\d+\.?\d*M)?(?:\d+\.?\d*D)?(?:T(?:{_NUM}H)?(?:{_NUM}M)?(?:{_NUM}S)?)?')


def duration_minutes(value: str):
    """The ``retentionTime`` rule (pyteomics' for ``xs:duration``), ``(minutes, None)`` or ``(None, reason)``: a
    value that does not begin with ``P`` is the numeral as written; an ISO-8601 duration is ``minutes + hours * 60.0
    + seconds / 60.0`` in that order, its years, months and days ignored; anything else, or a non-finite result, is
    refused. The device converts ``PT<seconds>S`` itself (``asl_mzxml_duration``: one division by 60.0) and hands
    every other form here."""
    if not value.startswith('P'):
        return _float(value.encode('utf-8'))
    m = _DURATION.fullmatch(value)
    if m is None or value == 'P' or value.endswith('T'):
        return None, f'{value!r} is not a duration'
    hours, minutes, seconds = (float(g) if g else 0.0 for g in m.groups())
    return minutes + hours * 60.0 + seconds / 60.0, None


class _Reader(QueryReader):
    PREFIX, RECORD, COUNT_KEY, ERR_TEXT, UNIT = 'mzXML: ', 'scan', 'n_spectra', _ERR_TEXT, b'<'

    def __init__(self, config, device, stats: Optional[dict], keep_raw: bool = False):
        super().__init__(config, device, stats, keep_raw)
        self.stats.update({'n_skipped_level': 0, 'n_skipped_id': 0, 'n_zlib': 0, 'n_arrays': 0, 'n_nested': 0})
        self.elem0 = 0                      # <scan tags of the file before the chunk: the next ``index``
        self.depth0 = 0                     # <scan> elements open in front of the chunk

    # ------------------------------------------------------------------ one chunk
    def measure(self, text: torch.Tensor, n: int, last: bool) -> np.ndarray:
        counts = np.zeros(16, np.int64)
        mode = int(last) | (2 if self.elem0 else 0) | (min(self.depth0, 255) << 8)
        _lib.check(_lib.lib().asl_mzxml_measure(_lib.ptr(text), n, mode, counts.ctypes.data_as(_lib.c_i64p)))
        return counts

    def before_chunk(self, buf: bytearray, consumed: int, counts: np.ndarray, last: bool) -> None:
        if last and counts[OPEN]:
            logging.warning('mzXML: the last scan is not closed at the end of the file: dropped')
        self.depth_next = int(counts[DEPTH_CONSUMED] if counts[OPEN] and not last else counts[DEPTH_ALL])

    def structural_errors(self, counts: np.ndarray) -> list:
        if not counts[ERR_KIND]:
            return []
        tag, elem = int(counts[ERR_LINE]), self.elem0 + int(counts[ERR_ELEMENT])
        where = f'scan {elem - 1}' if elem else 'before the first scan'
        return [(tag, 0, f'{where} (index; tag {self.line0 + tag + 1}): {self.ERR_TEXT[int(counts[ERR_KIND])]}')]

    def chunk(self, buf: bytearray, text: torch.Tensor, counts: np.ndarray, end_line: int) -> None:
        """Fill, check, sort and preprocess the MS2 scans of the measured chunk ``buf`` (``text`` on the device)
        whose heads are closed. ``end_line``: the tags of the chunk this call consumes."""
        dev, n = self.device, len(buf)
        ns, npk, n_elem = int(counts[N_RECORDS]), int(counts[N_PEAKS]), int(counts[N_ELEMENTS])
        errors = self.structural_errors(counts)
        self.stats['n_skipped_level'] += n_elem - ns
        if ns == 0:
            self._raise_first(errors)
            self.elem0 += n_elem
            self.depth0 = self.depth_next
            return
        t0 = time.perf_counter()
        offsets, mz, it, chg, pmz, _ = self.columns(ns, npk, 0)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        pz, ident, first, elem, num, err, flags, aerr = i32(ns), i32(ns, 2), i32(ns), i32(ns), i32(ns, 4), i32(ns), \
            i32(ns), i32(ns)
        rt = torch.empty(ns, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().asl_mzxml_fill(_lib.ptr(text), n, _lib.ptr(offsets), opt(mz), opt(it), opt(chg),
                                             opt(pmz), opt(pz), opt(rt), opt(ident), opt(first), opt(elem), opt(num),
                                             opt(err), opt(flags), opt(aerr)))
        pmz_h, pz_h, rt_h = pmz.cpu().numpy(), pz.cpu().numpy(), rt.cpu().numpy()
        ident_h, elem_h, num_h = ident.cpu().numpy(), elem.cpu().numpy(), num.cpu().numpy()
        err_h, flags_h, aerr_h = err.cpu().numpy(), flags.cpu().numpy(), aerr.cpu().numpy()
        behind = self.behind(first.cpu().numpy(), end_line)
        index = self.elem0 + elem_h.astype(np.int64)
        text_of = lambda o, l: unescape(bytes(buf[o:o + l]).decode('utf-8', 'replace'))
        # identifiers: Python's int() over num; the reference drops what it refuses, before it looks further
        raw_ids = [text_of(o, l) if l >= 0 else None for o, l in ident_h.tolist()]
        ids: List[Optional[str]] = []
        for r in raw_ids:
            try:
                ids.append(None if r is None else str(int(r)))
            except ValueError:
                ids.append(None)
        name = lambda s: f'scan {index[s]} (index; num {raw_ids[s]!r})'
        # the values the device deferred: durations and numerals
        for s, j in zip(*np.nonzero(num_h[:, 1::2] >= 0)):
            value = text_of(num_h[s, 2 * j], num_h[s, 2 * j + 1])
            v, why = duration_minutes(value) if j == 0 else _float(value.encode('utf-8'))
            if v is not None and not np.isfinite(v):
                v, why = None, f'non-finite {value!r}'
            if why and ids[s] is not None:
                errors.append((int(behind[s]), 1, f'{name(s)}: {("retentionTime", "precursor m/z")[j]} {why}'))
            (rt_h, pmz_h)[j][s] = 0.0 if why else v
        # what the device refused: first what fails while the reference iterates, then, for the scans whose
        # identifier is read, what fails in its parser
        no_id = np.array([r is None for r in raw_ids])
        bad_file = ((err_h & _E_FILE) != 0) | no_id | (aerr_h != 0)
        has_id = np.array([i is not None for i in ids])
        bad = bad_file | (has_id & (err_h != 0))
        for s in np.nonzero(bad)[0][:1]:
            if no_id[s]:
                why = 'no num attribute'
            elif bad_file[s] and (err_h[s] & _E_FILE) == 0:
                why = f'peaks: {_lib.MZML_INF_TEXT[int(aerr_h[s])]}'
            else:
                mask = _E_FILE if bad_file[s] else ~0
                why = next(t for b, t in _E_TEXT if err_h[s] & mask & b)
            errors.append((int(behind[s]), 1, f'{name(s)}: {why}'))
        self._raise_first(errors)
        for s in np.nonzero(~has_id)[0]:
            logging.warning('mzXML: failed to read scan %s: its num is not an integer', raw_ids[s])
        n_sorted = C.c_int64(0)
        _lib.check(_lib.lib().asl_mgf_sort(_lib.ptr(offsets), opt(mz), opt(it), ns, npk, C.byref(n_sorted)))
        raw = PackedSpectra(offsets, mz, it, chg, torch.as_tensor(pmz_h, device=dev),
                            torch.as_tensor(pz_h, device=dev))
        keep = np.nonzero(has_id)[0]
        if len(keep) < ns:
            raw = raw.select(torch.as_tensor(keep))
            pz_h, pmz_h, rt_h, index = pz_h[keep], pmz_h[keep], rt_h[keep], index[keep]
            ids = [ids[s] for s in keep]
        self._sync()
        t1 = time.perf_counter()
        if len(keep):
            self.take(raw, pz_h, pmz_h, rt_h, np.zeros(len(keep), bool), ids, index)
        st = self.stats
        st['n_skipped_id'] += ns - len(keep)
        st['n_arrays'] += ns
        st['n_zlib'] += int(np.count_nonzero(flags_h & _F_ZLIB))
        st['n_nested'] += int(np.count_nonzero(flags_h & _F_NESTED))
        self.account(t0, t1, ns, npk, 0, int(n_sorted.value))
        self.elem0 += n_elem
        self.depth0 = self.depth_next


def read_mzxml_raw(source, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The parse alone: ``(raw, retention_time, identifiers, index)`` -- the file's MS2 scans as one raw
    ``PackedSpectra`` on ``device`` (what ``library_store.pack_raw`` makes of the reader's objects: float32 peaks in
    file order, stably sorted by m/z where they descend; precursor charge 0 = unknown), the retention times in
    minutes (float64 numpy), the identifiers and the 0-based ordinals among all ``<scan`` opening tags. Arguments and
    errors as ``read_mzxml_packed``."""
    reader = _Reader(None, device, stats, keep_raw=True)
    reader.read_source(source, chunk_bytes)
    return reader.raw_result()


def read_mzxml_packed(source, config=None, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The MS2 scans of an mzXML file as ``library_store.pack_queries`` returns them for the reference's
    ``read_mzxml``: ``({charge: PackedSpectra}, {charge: [meta]})``, preprocessed, charges in order of first
    appearance, queries of unknown charge entered at 2 and 3, invalid spectra dropped, ``index`` the 0-based ordinal
    among the ``<scan`` opening tags of every MS level and nesting depth. ``source``: a path, or the file's bytes.
    The file is read in chunks of ``chunk_bytes``; the bytes behind the last closed head are carried into the next
    chunk, and a chunk that closes no head is doubled, up to ``text_reader.MAX_CHUNK``. ``stats``: a dict that
    receives what the reader counted: as ``mgf.read_mgf_packed`` (``n_lines``: tags), and ``n_skipped_level`` (scans
    of another MS level or without one), ``n_skipped_id`` (scans dropped, with a warning, because ``int()`` refuses
    their ``num``), ``n_arrays`` (streams decoded: one per MS2 scan), ``n_zlib`` (compressed ones) and ``n_nested``
    (MS2 scans whose head opened inside another scan's element). Deviations of the dialect raise ``ValueError``
    naming the scan by its ``index`` and ``num``, and for a decoding failure the reason; a scan of more than
    ``MAX_PEAKS`` peaks, or a tag of more than ``MAX_TAG`` bytes, raises ``AnnSoloMiError`` with ``code ==
    ERR_CAPACITY``. An unclosed last head is dropped with a warning."""
    reader = _Reader(config, device, stats)
    reader.read_source(source, chunk_bytes)
    return reader.result()
