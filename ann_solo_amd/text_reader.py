"""What the readers of record-structured text files share on the host (``mgf.py``, ``sptxt.py``, ``mzml.py``): the
chunk loop -- read, upload, measure, carry what the chunk does not close into the next one, double a chunk that closes
nothing -- and, per chunk, the tensors of a fill, the few numerals the device defers (Python's ``float``), the ranking
of the errors and the ``stats``. The device's side of the same split is ``csrc/text_records.hpp``. A "line" below is
the format's unit: a line behind a ``\\n`` or, for mzML, a tag at a ``<``.

A format subclasses ``ChunkedReader`` with its ``measure``, its ``chunk``, optionally ``before_chunk``, and the class
attributes below; everything about its dialect stays in its module. ``QueryReader`` adds what the query formats
(``mgf.py``, ``mzml.py``) share behind the parse: ``pack_queries`` from a chunk's raw pack on.
"""
import io
import math
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

MAX_CHUNK = (1 << 31) - 1           # bytes of one chunk: the ABI's limit

# counts[] of asl_mgf_measure and asl_sptxt_measure (N_RECORDS: ASL_MGF_N_SPECTRA)
N_LINES, N_RECORDS, N_PEAKS, N_DEFERRED, CONSUMED, CONSUMED_LINES, ERR_KIND, ERR_LINE, OPEN = range(9)
DEST_MZ, DEST_INTENSITY = range(2)  # the peak columns among a deferred token's destinations, in both ABIs


def _float(token: bytes):
    """(value, None) or (None, reason)."""
    try:
        v = float(token)
    except ValueError:
        return None, f'{token!r} is not a number'
    if not math.isfinite(v):
        return None, f'non-finite {token!r}'
    return v, None


def opt(a: torch.Tensor):
    return _lib.ptr(a) if a.numel() else None


class ChunkedReader:
    PREFIX = ''                     # of every message: 'MGF: '
    RECORD = ''                     # what does not fit a chunk: 'record' (its 1-based ordinal follows)
    COUNT_KEY = ''                  # the records' key in ``stats``: 'n_records'
    ERR_TEXT = {}                   # counts[ERR_KIND] -> message
    UNIT = b'\n'                    # the byte that delimits the units: a line starts behind it; any other byte (a
                                    # tag's b'<') starts its unit itself

    def __init__(self, device, stats: Optional[dict]):
        self.device = torch.device(device)
        self.timed = stats is not None      # only then are the parts synchronised for their timers
        self.stats = stats if stats is not None else {}
        self.stats.update({'chunks': 0, 'n_lines': 0, self.COUNT_KEY: 0, 'n_peaks': 0, 'n_deferred': 0,
                           'n_sorted': 0, 'grown': 0, 'read_s': 0.0, 'parse_s': 0.0, 'process_s': 0.0})
        self.line0 = 0                      # lines of the file before the chunk
        self.rec0 = 0                       # records of the file before the chunk

    # ------------------------------------------------------------------ the format's part
    def measure(self, text: torch.Tensor, n: int, last: bool) -> np.ndarray:
        """counts[] of the chunk ``text[:n]`` as the ABI defines them; returns synchronised."""
        raise NotImplementedError

    def chunk(self, buf: bytearray, text: torch.Tensor, counts: np.ndarray, end_line: int) -> None:
        """Take the closed records of the measured chunk ``buf`` (``text`` on the device). ``end_line``: the lines
        of the chunk this call consumes."""
        raise NotImplementedError

    def before_chunk(self, buf: bytearray, consumed: int, counts: np.ndarray, last: bool) -> None:
        """Called before ``chunk`` with the bytes of ``buf`` it consumes."""

    # ------------------------------------------------------------------ one chunk
    def _sync(self) -> None:
        """The timers of ``stats`` want finished work; without a caller's ``stats`` nothing waits here."""
        if self.timed and self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    def _raise_first(self, errors) -> None:
        """errors: (line or surrogate, 0 line-level | 1 record-level, message); the first in that order is raised."""
        if errors:
            raise ValueError(self.PREFIX + min(errors, key=lambda e: (e[0], e[1]))[2])

    def structural_errors(self, counts: np.ndarray) -> list:
        """The list of the chunk's errors, begun with the first one the device found."""
        if not counts[ERR_KIND]:
            return []
        ln = int(counts[ERR_LINE])
        return [(ln, 0, f'line {self.line0 + ln + 1}: {self.ERR_TEXT[int(counts[ERR_KIND])]}')]

    def columns(self, ns: int, npk: int, nd: int):
        """offsets, mz, intensity, charge, precursor_mz and the deferred records of a fill, on the device."""
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        return (new(ns + 1, torch.int32), new(npk, torch.float32), new(npk, torch.float32), new(npk, torch.uint8),
                new(ns, torch.float64), new((nd, 5), torch.int32))

    @staticmethod
    def behind(first_h: np.ndarray, end_line: int) -> np.ndarray:
        """Record-level errors stand at the line behind their record."""
        return np.append(first_h[1:], end_line).astype(np.int64)

    def patch_deferred(self, buf, rec: torch.Tensor, mz: torch.Tensor, it: torch.Tensor, none: int, errors: list,
                       on_record) -> None:
        """The few tokens the device defers: Python's ``float()``, stored before the sort and the pack. A peak's
        numeral goes to its slot of ``mz`` / ``it`` or, refused, to ``errors`` with its line; a record's goes to
        ``on_record(kind, index, value, why)``. Records of destination ``none`` name no winner: skipped."""
        slots = ([], []), ([], [])          # m/z, intensity: (peak slots, values)
        for o, l, kind, idx, ln in rec.cpu().numpy().tolist():
            if kind == none:
                continue
            v, why = _float(bytes(buf[o:o + l]))
            if kind > DEST_INTENSITY:
                on_record(kind, idx, v, why)
            elif why:
                errors.append((ln, 0, f'line {self.line0 + ln + 1}: {("m/z", "intensity")[kind]} {why}'))
            elif idx < mz.numel():          # (beyond: an unclosed last record, checked and dropped)
                slots[kind][0].append(idx)
                slots[kind][1].append(v)
        for (idx, values), column in zip(slots, (mz, it)):
            if idx:
                with np.errstate(over='ignore'):            # (a finite double beyond float32 is inf there)
                    v32 = np.asarray(values, np.float64).astype(np.float32)
                column[torch.as_tensor(idx, dtype=torch.int64, device=self.device)] = \
                    torch.as_tensor(v32, device=self.device)

    def account(self, t0: float, t1: float, ns: int, npk: int, nd: int, n_sorted: int) -> None:
        """A chunk's ``stats``: parsed from t0 to t1, processed since."""
        self._sync()
        st = self.stats
        st['parse_s'] += t1 - t0
        st['process_s'] += time.perf_counter() - t1
        st[self.COUNT_KEY] += ns
        st['n_peaks'] += npk
        st['n_deferred'] += nd
        st['n_sorted'] += n_sorted

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
            counts = self.measure(text, n, last)        # (returns synchronised)
            self.stats['read_s'] += t1 - t0
            self.stats['parse_s'] += time.perf_counter() - t1
            n_lines = int(counts[N_LINES])
            if last:
                consumed, end_line = n, n_lines
            elif counts[OPEN]:
                consumed, end_line = int(counts[CONSUMED]), int(counts[CONSUMED_LINES])
            elif self.UNIT == b'\n':
                if buf.endswith(b'\n'):     # no record is open: the chunk's whole lines
                    consumed, end_line = n, n_lines
                else:                       # a cut last line: it may be the start of a record
                    consumed, end_line = buf.rfind(b'\n') + 1, n_lines - 1
            else:                           # the last unit may be cut anywhere: it comes again with the next chunk
                cut = buf.rfind(self.UNIT)
                consumed, end_line = (n, n_lines) if cut < 0 else (cut, n_lines - 1)
            if consumed == 0 and not last:  # one record (or line) does not fit: a larger chunk
                if size >= MAX_CHUNK:
                    err = _lib.AnnSoloMiError(f'{self.PREFIX}{self.RECORD} {self.rec0 + 1} does not fit a chunk of '
                                              f'{MAX_CHUNK} bytes')
                    err.code = _lib.ERR_CAPACITY
                    raise err
                size = min(2 * size, MAX_CHUNK)
                self.stats['grown'] += 1
                del text
                continue
            self.before_chunk(buf, consumed, counts, last)
            self.chunk(buf, text, counts, end_line)
            self.stats['chunks'] += 1
            self.stats['n_lines'] += end_line
            self.line0 += end_line
            self.rec0 += int(counts[N_RECORDS])
            del text
            del buf[:consumed]
            if last:
                break

    def read_source(self, source, chunk_bytes: int) -> None:
        """``source``: a path, or the file's bytes."""
        if isinstance(source, (str, os.PathLike)):
            with open(source, 'rb') as f:
                self.read(f, chunk_bytes)
        else:
            self.read(io.BytesIO(bytes(source)), chunk_bytes)


PROCESS_ROWS = 1 << 17              # spectra per ``process_spectra`` call


class QueryReader(ChunkedReader):
    """A reader of query files: its ``chunk`` hands every chunk's raw pack to ``take``, which keeps it
    (``keep_raw``: the parse alone) or preprocesses it as ``library_store.pack_queries`` does."""

    def __init__(self, config, device, stats: Optional[dict], keep_raw: bool = False):
        from .config import Config
        super().__init__(device, stats)
        self.config = Config.from_reference(config)
        self.raw = [] if keep_raw else None     # the chunks' raw packs instead of the preprocessing
        self.pieces: Dict[int, List] = {}
        self.metas: Dict[int, List[dict]] = {}

    def take(self, raw, pz_h, pmz_h, rt_h, rt_none, ids, index) -> None:
        if self.raw is not None:
            self.raw.append((raw, np.where(rt_none, np.nan, rt_h), ids, np.asarray(index)))
        else:
            self._preprocess(raw, pz_h, pmz_h, rt_h, rt_none, ids, index)

    def _preprocess(self, raw, pz_h, pmz_h, rt_h, rt_none, ids, index) -> None:
        """``pack_queries`` from the raw pack on: unknown charges entered at 2 and 3, ``process_spectra``, the
        invalid copies dropped, rows and meta records appended per charge. ``index``: the spectra's ``index``."""
        from .packed import PackedSpectra
        from .spectrum import process_spectra
        ns = raw.n
        unknown = pz_h == 0
        reps = np.where(unknown, 2, 1)
        rows = np.repeat(np.arange(ns), reps)
        z = np.repeat(pz_h, reps).astype(np.int32)
        if unknown.any():
            second = np.r_[False, rows[1:] == rows[:-1]]
            z = np.where(np.repeat(unknown, reps), np.where(second, 3, 2), z).astype(np.int32)
        for a in range(0, len(rows), PROCESS_ROWS):
            r, zz = rows[a:a + PROCESS_ROWS], z[a:a + PROCESS_ROWS]
            part = raw if (len(r) == ns and not unknown.any()) else raw.select(torch.as_tensor(r))
            part = PackedSpectra(part.offsets, part.mz, part.intensity, part.charge, part.precursor_mz,
                                 torch.as_tensor(zz, device=self.device))
            out, valid = process_spectra(part, False, self.config, self.device)
            ok = valid.cpu().numpy()
            keep = np.nonzero(ok)[0]
            _, first_at = np.unique(zz[keep], return_index=True)
            for j in np.sort(first_at):                   # charges in order of first appearance
                c = int(zz[keep[j]])
                sel = keep[zz[keep] == c]
                self.pieces.setdefault(c, []).append(out.select(torch.as_tensor(sel)).to('cpu'))
                meta = self.metas.setdefault(c, [])
                for s in r[sel].tolist():
                    meta.append(dict(identifier=ids[s], index=int(index[s]),
                                     retention_time=None if rt_none[s] else float(rt_h[s]),
                                     precursor_charge=c, precursor_mz=float(pmz_h[s])))

    def result(self):
        from .library_store import concat_packs
        from .packed import PackedSpectra
        packs = {}
        for c, meta in self.metas.items():
            p = concat_packs(self.pieces[c])
            packs[c] = PackedSpectra(p.offsets, p.mz, p.intensity, p.charge, p.precursor_mz, p.precursor_charge,
                                     identifiers=[m['identifier'] for m in meta])
        return packs, self.metas

    def raw_result(self):
        """``(raw, retention_time, identifiers, index)`` of a ``keep_raw`` reader."""
        from .library_store import concat_packs
        from .packed import PackedSpectra
        if not self.raw:
            z = lambda dt: torch.zeros(0, dtype=dt, device=self.device)
            return (PackedSpectra(torch.zeros(1, dtype=torch.int32, device=self.device), z(torch.float32),
                                  z(torch.float32), z(torch.uint8), z(torch.float64), z(torch.int32)),
                    np.zeros(0, np.float64), [], np.zeros(0, np.int64))
        return (concat_packs([r[0] for r in self.raw]), np.concatenate([r[1] for r in self.raw]),
                [i for r in self.raw for i in r[2]], np.concatenate([r[3] for r in self.raw]).astype(np.int64))
