"""The chunk loop the text readers share (``text_reader.ChunkedReader.read``), on the CPU and without the library: a
toy format measured in plain Python. A record is the lines from a ``B`` line to the next ``E`` line; ``measure``
returns counts[] as the ABI defines them for a chunk (annsolo_mi.h, asl_mgf_measure): the lines, the closed records,
the byte and the lines behind the last closed record, whether the chunk ends inside a record; a final line without
its line end is not looked at unless the chunk ends the file."""
import io

import numpy as np
import pytest

from ann_solo_amd import _lib, text_reader
from ann_solo_amd.text_reader import CONSUMED, CONSUMED_LINES, ERR_LINE, N_LINES, N_RECORDS, OPEN, ChunkedReader


def toy_lines(data: bytes, last: bool):
    lines = data.splitlines(keepends=True)
    return lines, [l.strip() if last or l.endswith(b'\n') else b'' for l in lines]     # (a cut line: not looked at)


class ToyReader(ChunkedReader):
    PREFIX, RECORD, COUNT_KEY = 'toy: ', 'unit', 'n_units'

    def __init__(self):
        super().__init__('cpu', None)
        self.records, self.calls = [], []

    def measure(self, text, n, last):
        data = bytes(text.numpy()[:n])
        counts = np.zeros(16, np.int64)
        lines, heads = toy_lines(data, last)
        inside, pos = False, 0
        for i, (line, head) in enumerate(zip(lines, heads)):
            pos += len(line)
            if not inside and head == b'B':
                inside = True
            elif inside and head == b'E':
                inside = False
                counts[N_RECORDS] += 1
                counts[CONSUMED], counts[CONSUMED_LINES] = pos, i + 1
        counts[N_LINES], counts[OPEN], counts[ERR_LINE] = len(lines), int(inside), -1
        return counts

    def before_chunk(self, buf, consumed, counts, last):
        self.calls.append(dict(n=len(buf), consumed=consumed, last=last, line0=self.line0, rec0=self.rec0))

    def chunk(self, buf, text, counts, end_line):
        call = self.calls[-1]
        taken = bytes(buf[:call['consumed']])
        assert taken.count(b'\n') + (not taken.endswith(b'\n')) == end_line
        lines, heads = toy_lines(taken, call['last'])
        start = None
        for i, head in enumerate(heads):
            if start is None and head == b'B':
                start = i
            elif start is not None and head == b'E':
                self.records.append(b''.join(lines[start:i + 1]))
                start = None
        assert len(self.records) == self.rec0 + int(counts[N_RECORDS])


def toy_file(between: bool, seed: int = 5):
    """About 20 records of 0 .. 12 payload lines; ``between``: lines outside the records too, and a preamble."""
    rng = np.random.default_rng(seed)
    parts, records = ([b'# toy\n', b'\n'] if between else []), []
    for r in range(20):
        k = 30 if r == 11 else int(rng.integers(1 if r == 14 else 0, 13))
        rec = b'B\n' + b''.join(b'%d.%d %s\n' % (r, j, b'x' * int(rng.integers(0, 9))) for j in range(k)) + b'E\n'
        records.append(rec)
        parts.append(rec)
        if between and r % 3 == 0:
            parts.append(b'between %d\n' % r)
    data = b''.join(parts)
    assert len(data) < 2048
    return data, records


def n_lines_of(data: bytes) -> int:
    return data.count(b'\n') + (1 if data and not data.endswith(b'\n') else 0)


def read(data: bytes, chunk_bytes: int) -> ToyReader:
    reader = ToyReader()
    reader.read(io.BytesIO(data), chunk_bytes)
    return reader


@pytest.mark.parametrize('between', [False, True])
def test_every_chunk_size_gives_the_records_in_order(between):
    data, records = toy_file(between)
    longest = max(len(r) for r in records)
    for c in range(1, len(data) + 2):
        reader = read(data, c)
        assert reader.records == records, c
        st = reader.stats
        assert st['n_lines'] == reader.line0 == n_lines_of(data), c
        assert reader.rec0 == len(records) and st['chunks'] == len(reader.calls), c
        done = 0
        for call in reader.calls:           # line0 and the ordinal advance by what each chunk consumed
            assert call['line0'] == data[:done].count(b'\n'), c
            assert 0 < call['consumed'] <= call['n'] or call['last'], c
            done += call['consumed']
        assert done == len(data), c
        if not between:                     # every chunk starts at a record: only a record can fail to fit
            assert (st['grown'] > 0) == (longest > c), c


def test_record_ordinals_advance_with_the_records_taken():
    data, records = toy_file(False)
    starts = np.cumsum([0] + [len(r) for r in records])
    for c in (1, 7, 64, 300, len(data)):
        done = 0
        for call in read(data, c).calls:
            assert call['rec0'] == int(np.searchsorted(starts, done)), c       # (consumed ends at a record's end)
            done += call['consumed']


def test_a_record_beyond_the_largest_chunk_is_a_capacity_error(monkeypatch):
    data, records = toy_file(False)
    sizes = [len(r) for r in records]
    monkeypatch.setattr(text_reader, 'MAX_CHUNK', max(sizes) - 1)
    with pytest.raises(_lib.AnnSoloMiError) as e:
        read(data, 16)
    assert e.value.code == _lib.ERR_CAPACITY
    assert str(e.value) == f'toy: unit {int(np.argmax(sizes)) + 1} does not fit a chunk of {max(sizes) - 1} bytes'
    with pytest.raises(ValueError, match='at most'):
        read(data, max(sizes))
    monkeypatch.setattr(text_reader, 'MAX_CHUNK', max(sizes))                 # it fits: doubled up to the limit
    assert read(data, 16).records == records


@pytest.mark.parametrize('between', [False, True])
def test_a_file_cut_inside_a_line_of_a_record_is_consumed_by_the_last_call(between):
    full, records = toy_file(between)
    data = full[:full.index(records[14]) + records[14].rindex(b'14.') + 4]    # inside its last payload line
    assert data.rsplit(b'\n', 1)[1][:3] == b'14.'
    for c in range(1, len(data) + 2):
        reader = read(data, c)
        assert reader.records == records[:14], c
        final = reader.calls[-1]
        assert final['last'] and final['consumed'] == final['n'], c
        assert [call['last'] for call in reader.calls[:-1]] == [False] * (len(reader.calls) - 1), c
        assert sum(call['consumed'] for call in reader.calls) == len(data), c
        assert reader.stats['n_lines'] == reader.line0 == n_lines_of(data), c
