"""mzML query files read on the device (``Config.device_mzml``; DESIGN.md 3 "Query files").

``read_mzml_packed(source, config, device)`` returns what ``library_store.pack_queries`` returns for the MS2
spectra the reference's ``read_mzml`` yields from an mzML file -- the same charges in the same order, the same
tensors bit for bit, the same meta records -- without pyteomics, lxml, or a Python object per spectrum: the text is
uploaded in chunks, split into tags, classified, and its base64 / zlib arrays decoded by the kernels of
``csrc/mzml.hip`` and ``csrc/inflate.hpp`` (``asl_mzml_measure`` / ``asl_mzml_fill``, then ``asl_mgf_sort``), and the
raw pack goes to the existing ``process_spectra`` where it lies. The host's part: the identifiers (the reference's
``scan=`` / ``index=`` rule, with Python's own ``int``), the few numerals the device defers (Python's ``float``),
the error codes turned into ``ValueError`` and the meta records. The chunk loop is ``text_reader.ChunkedReader``,
what follows the parse ``text_reader.QueryReader``, both shared with ``mgf.py``.

The dialect is stated in ``include/annsolo_mi.h`` and restated in ``tests/mzml_ref.py``. pyteomics is not a
dependency: the statement is unpinned, like the MGF reader's.
"""
import ctypes as C
import logging
import re
import time
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .packed import PackedSpectra
from .text_reader import ERR_KIND, ERR_LINE, N_PEAKS, N_RECORDS, OPEN, QueryReader, _float, opt

SCAN_TILE = _lib.MGF_TILE               # tags per workgroup of the reader's scans (ASL_MGF_TILE)
MAX_PEAKS = _lib.MGF_MAX_PEAKS          # defaultArrayLength of one spectrum (ASL_MGF_MAX_PEAKS)
MAX_TAG = _lib.MZML_MAX_TAG             # bytes of one tag (ASL_MZML_MAX_TAG)
SMALL_PEAKS = _lib.MZML_SMALL_PEAKS     # the decode kernel's size classes (ASL_MZML_SMALL_PEAKS)

N_ELEMENTS, ERR_ELEMENT = 9, 10         # counts[] of asl_mzml_measure behind the shared ones
_ERR_TEXT = {1: 'a <spectrum> inside a <spectrum>', 2: 'a comment or CDATA section after the first <spectrum',
             3: 'a tag that does not end'}
# errors[] of asl_mzml_fill (ASL_MZML_E_*)
_E_FILE = 0x7f
_E_TEXT = [(0x1, 'defaultArrayLength is missing or not a number'), (0x2, 'no m/z array'),
           (0x4, 'no intensity array'), (0x8, 'a missing or unsupported precision (64- or 32-bit float)'),
           (0x10, 'a missing or unsupported compression (none or zlib)'),
           (0x20, 'an arrayLength attribute on a binaryDataArray'), (0x40, 'a referenceableParamGroupRef'),
           (0x100, 'no scan start time'), (0x200, 'no precursor with a selected ion m/z'),
           (0x400, 'several possible charge states'), (0x800, 'a charge that is not a number in 1 .. 255')]

_ENTITY = re.compile(r'&(#[0-9]+|#x[0-9a-fA-F]+|lt|gt|amp|quot|apos);')
_NAMED = {'lt': '<', 'gt': '>', 'amp': '&', 'quot': '"', 'apos': "'"}


def _entity(m) -> str:
    e = m.group(1)
    if e[0] != '#':
        return _NAMED[e]
    return chr(int(e[2:], 16) if e[1] == 'x' else int(e[1:]))


def unescape(value: str) -> str:
    """An attribute value with its character and entity references resolved."""
    return _ENTITY.sub(_entity, value) if '&' in value else value


def scan_identifier(spectrum_id: str) -> Optional[str]:
    """The reference's identifier of a spectrum id (reader.py ``_parse_spectrum_mzml``): the integer behind the
    first ``scan=``, else behind the first ``index=``, as a string; None where the reference raises the
    ``ValueError`` it catches (neither form, or a tail ``int()`` refuses)."""
    for key in ('scan=', 'index='):
        if key in spectrum_id:
            try:
                return str(int(spectrum_id[spectrum_id.find(key) + len(key):]))
            except ValueError:
                return None
    return None


class _Reader(QueryReader):
    PREFIX, RECORD, COUNT_KEY, ERR_TEXT, UNIT = 'mzML: ', 'spectrum', 'n_spectra', _ERR_TEXT, b'<'

    def __init__(self, config, device, stats: Optional[dict], keep_raw: bool = False):
        super().__init__(config, device, stats, keep_raw)
        self.stats.update({'n_skipped_level': 0, 'n_skipped_id': 0, 'n_zlib': 0, 'n_arrays': 0, 'n_small': 0})
        self.elem0 = 0                      # <spectrum> elements of the file before the chunk: the next ``index``

    # ------------------------------------------------------------------ one chunk
    def measure(self, text: torch.Tensor, n: int, last: bool) -> np.ndarray:
        counts = np.zeros(16, np.int64)
        _lib.check(_lib.lib().asl_mzml_measure(_lib.ptr(text), n, int(last) | (2 if self.elem0 else 0),
                                               counts.ctypes.data_as(_lib.c_i64p)))
        return counts

    def before_chunk(self, buf: bytearray, consumed: int, counts: np.ndarray, last: bool) -> None:
        if last and counts[OPEN]:
            logging.warning('mzML: the last spectrum is not closed at the end of the file: dropped')

    def structural_errors(self, counts: np.ndarray) -> list:
        if not counts[ERR_KIND]:
            return []
        tag, elem = int(counts[ERR_LINE]), self.elem0 + int(counts[ERR_ELEMENT])
        where = f'spectrum {elem - 1}' if elem else 'before the first spectrum'
        return [(tag, 0, f'{where} (index; tag {self.line0 + tag + 1}): {self.ERR_TEXT[int(counts[ERR_KIND])]}')]

    def chunk(self, buf: bytearray, text: torch.Tensor, counts: np.ndarray, end_line: int) -> None:
        """Fill, check, sort and preprocess the closed MS2 spectra of the measured chunk ``buf`` (``text`` on the
        device). ``end_line``: the tags of the chunk this call consumes."""
        dev, n = self.device, len(buf)
        ns, npk, n_elem = int(counts[N_RECORDS]), int(counts[N_PEAKS]), int(counts[N_ELEMENTS])
        errors = self.structural_errors(counts)
        self.stats['n_skipped_level'] += n_elem - ns
        if ns == 0:
            self._raise_first(errors)
            self.elem0 += n_elem
            return
        t0 = time.perf_counter()
        offsets, mz, it, chg, pmz, _ = self.columns(ns, npk, 0)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        pz, ident, first, elem, num, err, flags, aerr = i32(ns), i32(ns, 2), i32(ns), i32(ns), i32(ns, 4), i32(ns), \
            i32(ns), i32(ns, 2)
        rt = torch.empty(ns, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().asl_mzml_fill(_lib.ptr(text), n, _lib.ptr(offsets), opt(mz), opt(it), opt(chg),
                                            opt(pmz), opt(pz), opt(rt), opt(ident), opt(first), opt(elem), opt(num),
                                            opt(err), opt(flags), opt(aerr)))
        pmz_h, pz_h, rt_h = pmz.cpu().numpy(), pz.cpu().numpy(), rt.cpu().numpy()
        ident_h, elem_h, num_h = ident.cpu().numpy(), elem.cpu().numpy(), num.cpu().numpy()
        err_h, flags_h, aerr_h = err.cpu().numpy(), flags.cpu().numpy(), aerr.cpu().numpy()
        behind = self.behind(first.cpu().numpy(), end_line)
        index = self.elem0 + elem_h.astype(np.int64)
        # identifiers: the reference drops what its rule refuses, before it looks at the parameters
        raw_ids = [unescape(bytes(buf[o:o + l]).decode('utf-8')) if l >= 0 else None for o, l in ident_h.tolist()]
        ids: List[Optional[str]] = [None if r is None else scan_identifier(r) for r in raw_ids]
        name = lambda s: f'spectrum {index[s]} (index; id {raw_ids[s]!r})'
        # the numerals the device deferred
        for s, j in zip(*np.nonzero(num_h[:, 1::2] >= 0)):
            o, l = num_h[s, 2 * j], num_h[s, 2 * j + 1]
            v, why = _float(unescape(bytes(buf[o:o + l]).decode('utf-8')).encode('utf-8'))
            if why and ids[s] is not None:
                errors.append((int(behind[s]), 1, f'{name(s)}: {("scan start time", "selected ion m/z")[j]} {why}'))
            (rt_h, pmz_h)[j][s] = 0.0 if why else v
        # what the device refused: first what fails while the reference iterates, then, for the spectra whose
        # identifier is read, what fails in its parser
        no_id = np.array([r is None for r in raw_ids])
        bad_file = ((err_h & _E_FILE) != 0) | no_id | (aerr_h != 0).any(axis=1)
        has_id = np.array([i is not None for i in ids])
        bad = bad_file | (has_id & (err_h != 0))
        for s in np.nonzero(bad)[0][:1]:
            if no_id[s]:
                why = 'no id attribute'
            elif bad_file[s] and (err_h[s] & _E_FILE) == 0:
                j = int(np.argmax(aerr_h[s] != 0))
                why = f'{("m/z", "intensity")[j]} array: {_lib.MZML_INF_TEXT[int(aerr_h[s, j])]}'
            else:
                mask = _E_FILE if bad_file[s] else ~0
                why = next(t for b, t in _E_TEXT if err_h[s] & mask & b)
            errors.append((int(behind[s]), 1, f'{name(s)}: {why}'))
        self._raise_first(errors)
        for s in np.nonzero(~has_id)[0]:
            logging.warning('mzML: failed to read spectrum %s: no scan or index number in its id', raw_ids[s])
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
        st['n_arrays'] += 2 * ns
        st['n_zlib'] += int(np.count_nonzero(flags_h & 0x1) + np.count_nonzero(flags_h & 0x4))
        st['n_small'] += 2 * int(np.count_nonzero(np.diff(offsets.cpu().numpy()) <= SMALL_PEAKS))
        self.account(t0, t1, ns, npk, 0, int(n_sorted.value))
        self.elem0 += n_elem


def read_mzml_raw(source, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The parse alone: ``(raw, retention_time, identifiers, index)`` -- the file's MS2 spectra as one raw
    ``PackedSpectra`` on ``device`` (what ``library_store.pack_raw`` makes of the reader's objects: float32 peaks in
    file order, stably sorted by m/z where they descend; precursor charge 0 = unknown), the retention times
    (float64 numpy), the identifiers and the 0-based ordinals among all ``<spectrum>`` elements. Arguments and
    errors as ``read_mzml_packed``."""
    reader = _Reader(None, device, stats, keep_raw=True)
    reader.read_source(source, chunk_bytes)
    return reader.raw_result()


def read_mzml_packed(source, config=None, device='cuda', chunk_bytes: int = 256 << 20, stats: Optional[dict] = None):
    """The MS2 spectra of an mzML file as ``library_store.pack_queries`` returns them for the reference's
    ``read_mzml``: ``({charge: PackedSpectra}, {charge: [meta]})``, preprocessed, charges in order of first
    appearance, queries of unknown charge entered at 2 and 3, invalid spectra dropped, ``index`` the 0-based ordinal
    among the ``<spectrum>`` elements of every MS level. ``source``: a path, or the file's bytes. The file is read in
    chunks of ``chunk_bytes``; the bytes behind the last closed ``</spectrum>`` are carried into the next chunk, and
    a chunk that closes no spectrum is doubled, up to ``text_reader.MAX_CHUNK``. ``stats``: a dict that receives
    what the reader counted: as ``mgf.read_mgf_packed`` (``n_lines``: tags), and ``n_skipped_level`` (spectra of
    another MS level), ``n_skipped_id`` (spectra dropped, with a warning, because their id has neither ``scan=`` nor
    ``index=`` with an integer behind it), ``n_arrays``, ``n_zlib`` (compressed ones) and ``n_small`` (arrays of the
    decode kernel's small size class). Deviations of the dialect raise ``ValueError`` naming the spectrum by its
    ``index`` and id, and for a decoding failure the array; a spectrum of more than ``MAX_PEAKS`` peaks, or a tag of
    more than ``MAX_TAG`` bytes, raises ``AnnSoloMiError`` with ``code == ERR_CAPACITY``. An unclosed last spectrum
    is dropped with a warning."""
    reader = _Reader(config, device, stats)
    reader.read_source(source, chunk_bytes)
    return reader.result()
