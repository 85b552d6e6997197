"""The preprocessing kernel (csrc/process.hip) on the named edge cases of process_cases -- the three
sort sizes at their boundaries, max_peaks 1 and 256, ties at the cut-off, the threshold and validity
equalities, merge runs of a thousand peaks, precursor removal at its tolerance, zero / infinite / NaN
intensities -- under the contract of test_gpu_process.test_process_matches_oracle (validity equal, m/z
equal, intensities BIT-equal, annotations following their peaks, nothing for an invalid spectrum), and
the host paths of asl_process_batch no other test runs: host pointers, out_src == NULL, the capacity
error of a spectrum above 4096 peaks and the argument checks."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from process_cases import CASES, Case, NAN_NEG, cfg_key, config_attrs, oracle_args

pytestmark = pytest.mark.gpu

# neighbours put between the cases of every batch: empty, nothing inside the m/z window, all NaN
_FILLERS = [
    ('filler_empty', np.zeros(0, np.float32), np.zeros(0, np.float32)),
    ('filler_out_of_range', np.linspace(1, 10, 12).astype(np.float32), np.ones(12, np.float32)),
    ('filler_all_nan', np.linspace(100, 1900, 40).astype(np.float32), np.full(40, NAN_NEG, np.float32)),
]


def _groups():
    """One batch per cfg: its cases, a filler after each."""
    by_cfg = {}
    for c in CASES:
        by_cfg.setdefault(cfg_key(c.cfg), []).append(c)
    out, k = [], 0
    for key, cases in by_cfg.items():
        batch = []
        for c in cases:
            name, mz, it = _FILLERS[k % len(_FILLERS)]
            k += 1
            batch += [c, Case(name, mz, it, np.zeros(len(mz), np.uint8), 600.0, 2, c.cfg, dict(valid=False))]
        out.append(batch)
    return out


GROUPS = _groups()
_ids = [g[0].name + '+%d' % (len(g) // 2 - 1) for g in GROUPS]


def _pack(cases):
    from ann_solo_amd.packed import PackedSpectra
    offs = np.concatenate([[0], np.cumsum([len(c.mz) for c in cases])])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False) if xs else np.zeros(0, dt)
    return PackedSpectra.from_numpy(offs, cat([c.mz for c in cases], np.float32),
                                    cat([c.intensity for c in cases], np.float32),
                                    cat([c.charge for c in cases], np.uint8),
                                    np.array([c.precursor_mz for c in cases]),
                                    np.array([c.precursor_charge for c in cases]))


def _run(cases, device='cuda'):
    """process_spectra over one batch -> per spectrum (valid, mz, intensity bits, annotations)."""
    from ann_solo_amd import spectrum
    out, valid = spectrum.process_spectra(_pack(cases), False,
                                          SimpleNamespace(**config_attrs(cases[0].cfg)), device=device)
    o, mz, it, chg, _, _ = out.to('cpu').numpy()
    valid = valid.cpu().numpy()
    assert len(valid) == len(cases) == len(o) - 1
    return [(bool(valid[s]), mz[o[s]:o[s + 1]].copy(), it[o[s]:o[s + 1]].view(np.uint32).copy(),
             chg[o[s]:o[s + 1]].copy()) for s in range(len(cases))]


_CACHE = {}


def _batch(g):
    """The device-tensor result of batch ``g``, computed once and shared."""
    if g not in _CACHE:
        _CACHE[g] = _run(GROUPS[g])
    return _CACHE[g]


def _oracle(O, c):
    key = ('oracle', c.name, cfg_key(c.cfg))
    if key not in _CACHE:
        _CACHE[key] = O.process_spectrum(c.mz, c.intensity, c.precursor_mz, c.precursor_charge,
                                         **oracle_args(c.cfg))
    return _CACHE[key]


def _check(O, c, got):
    ok, rm, ri, rs = _oracle(O, c)
    valid, mz, bits, chg = got
    assert valid == ok, c.name
    if not ok:
        assert len(mz) == 0 and len(bits) == 0, c.name
        return
    assert np.array_equal(mz, rm), c.name
    assert np.array_equal(bits, ri.view(np.uint32)), c.name
    assert np.array_equal(chg, c.charge[rs]), c.name          # annotations follow their peaks


def _same(a, b, what):
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), what


def test_every_case_is_run():
    ran = [c.name for g in GROUPS for c in g if not c.name.startswith('filler_')]
    assert sorted(ran) == sorted(c.name for c in CASES)
    assert all(len({cfg_key(c.cfg) for c in g}) == 1 for g in GROUPS)


@pytest.mark.parametrize('g', range(len(GROUPS)), ids=_ids)
def test_batch_matches_oracle(O, g):
    got = _batch(g)
    for c, r in zip(GROUPS[g], got):
        _check(O, c, r)
    assert any(r[0] for r in got) or not any(c.exp['valid'] for c in GROUPS[g])


@pytest.mark.parametrize('g', range(len(GROUPS)), ids=_ids)
def test_alone_matches_oracle_and_batch(O, g):
    """n = 1: the same result as inside the batch, whatever the neighbours were."""
    got = _batch(g)
    for c, r in zip(GROUPS[g], got):
        if c.name.startswith('filler_') and c.name != 'filler_empty':
            continue
        alone = _run([c])[0]
        _check(O, c, alone)
        _same(alone, r, c.name)


@pytest.mark.parametrize('g', range(len(GROUPS)), ids=_ids)
def test_host_pointers_match_device_tensors(g):
    """device='cpu': every array is a host pointer the library stages itself."""
    host = _run(GROUPS[g], device='cpu')
    for c, a, b in zip(GROUPS[g], host, _batch(g)):
        _same(a, b, c.name)


def _params(cfg):
    from ann_solo_amd import _lib
    res = cfg.get('resolution')
    return _lib.AslProcessParams(
        11.0, 2010.0, int(cfg.get('remove_precursor', False)), float(cfg.get('rp_tol', 0.0)),
        float(cfg.get('min_intensity', 0.01)), int(cfg.get('max_peaks', 50)),
        {'rank': 1, 'sqrt': 2, None: 0}[cfg.get('scaling', 'rank')], int(cfg.get('min_peaks', 10)),
        float(cfg.get('min_mz_range', 250.0)), int(res is not None), int(res or 0))


def _call(raw, P, with_src=True, device='cuda'):
    """asl_process_batch itself -> (return code, out_mz, out_intensity bits, out_src, count, valid)."""
    from ann_solo_amd import _lib
    r = raw.to(device).contiguous()
    n, mp = r.n, P.max_peaks
    o_mz = torch.zeros((n, mp), dtype=torch.float32, device=device)
    o_in = torch.zeros((n, mp), dtype=torch.float32, device=device)
    o_src = torch.zeros((n, mp), dtype=torch.int32, device=device)
    o_cnt = torch.zeros(n, dtype=torch.int32, device=device)
    o_val = torch.zeros(n, dtype=torch.uint8, device=device)
    rc = _lib.lib().asl_process_batch(C.byref(_lib.peaks_struct(r)), C.byref(P), _lib.ptr(o_mz),
                                      _lib.ptr(o_in), _lib.ptr(o_src) if with_src else None,
                                      _lib.ptr(o_cnt), _lib.ptr(o_val))
    return (rc, o_mz.cpu().numpy(), o_in.cpu().numpy().view(np.uint32), o_src.cpu().numpy(),
            o_cnt.cpu().numpy(), o_val.cpu().numpy())


def _first_group(pred):
    return next(g for g in GROUPS if pred(g[0].cfg))


@pytest.mark.parametrize('device', ['cuda', 'cpu'])
@pytest.mark.parametrize('group', [
    _first_group(lambda c: c == {}),
    _first_group(lambda c: c.get('resolution') == 0),
    _first_group(lambda c: c.get('max_peaks') == 256 and c.get('scaling') == 'sqrt'),
], ids=['defaults', 'rounded', 'max_peaks_256'])
def test_out_src_null(group, device):
    """out_src == NULL (the library's own temporary): everything else as with the pointer. Compared are
    the slots the call defines, the first out_count[s] of a row (include/annsolo_mi.h)."""
    raw, P = _pack(group), _params(group[0].cfg)
    a = _call(raw, P, True, device)
    b = _call(raw, P, False, device)
    assert a[0] == 0 and b[0] == 0
    assert a[5].any() and not a[5].all()
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    assert ((a[4] > 0) == (a[5] != 0)).all() and a[4].max() <= P.max_peaks
    slot = np.arange(P.max_peaks)[None, :] < a[4][:, None]
    assert np.array_equal(a[1][slot], b[1][slot]) and np.array_equal(a[2][slot], b[2][slot])
    assert (np.diff(a[3], axis=1)[slot[:, 1:]] > 0).all()     # source indices ascend inside a row
    assert not b[3].any()                                     # the caller's buffer was not touched


def test_spectrum_above_4096_peaks_fails_the_call_only(O):
    """One raw spectrum of 4097 peaks: the whole call raises the capacity error (callers split or
    pre-filter); the status word does not leak into the next call."""
    from ann_solo_amd import _lib
    g = GROUPS.index(_first_group(lambda c: c == {}))
    rng = np.random.default_rng(5)
    long = Case('long', np.sort(rng.uniform(11, 2010, 4097)).astype(np.float32),
                rng.uniform(1, 2, 4097).astype(np.float32), np.zeros(4097, np.uint8), 600.0, 2, {},
                dict(valid=False))
    batch = GROUPS[g][:3] + [long] + GROUPS[g][3:]
    for device in ('cuda', 'cpu'):
        with pytest.raises(_lib.AnnSoloMiError, match='4096') as e:
            _run(batch, device=device)
        assert e.value.code == _lib.ERR_CAPACITY
        after = _run(GROUPS[g], device=device)
        for c, a, b in zip(GROUPS[g], after, _batch(g)):
            _check(O, c, a)
            _same(a, b, c.name)


def test_argument_checks():
    from ann_solo_amd import _lib
    L = _lib.lib()
    group = _first_group(lambda c: c == {})
    raw = _pack(group).to('cuda')
    S = _lib.peaks_struct(raw)
    n = raw.n
    o_mz = torch.zeros((n, 256), dtype=torch.float32, device='cuda')
    o_in, o_src = torch.zeros_like(o_mz), torch.zeros((n, 256), dtype=torch.int32, device='cuda')
    o_cnt = torch.zeros(n, dtype=torch.int32, device='cuda')
    o_val = torch.zeros(n, dtype=torch.uint8, device='cuda')
    outs = [_lib.ptr(t) for t in (o_mz, o_in, o_src, o_cnt, o_val)]

    def call(P=None, raw_=True, p_=True, outs_=outs):
        P = P if P is not None else _params({})
        return L.asl_process_batch(C.byref(S) if raw_ else None, C.byref(P) if p_ else None, *outs_)
    assert call() == 0 and int(o_val.sum()) > 0
    for cfg in (dict(max_peaks=0), dict(max_peaks=257), dict(resolution=-7), dict(resolution=13)):
        assert call(_params(cfg)) == _lib.ERR_INVALID, cfg
        assert L.asl_last_error()
    assert call(_params(dict(resolution=-6, min_peaks=1, min_mz_range=0.0))) == 0
    assert call(_params(dict(resolution=12))) == 0
    P = _params({})
    P.resolution = 13                                          # not read while rounding is off
    assert call(P) == 0
    assert call(raw_=False) == _lib.ERR_INVALID
    assert call(p_=False) == _lib.ERR_INVALID
    for k in (0, 1, 3, 4):                                     # out_mz, out_intensity, out_count, out_valid
        assert call(outs_=outs[:k] + [None] + outs[k + 1:]) == _lib.ERR_INVALID, k
    empty = _lib.AslPeaks(0, None, None, None, None, None, None, 0)
    assert L.asl_process_batch(C.byref(empty), C.byref(_params({})), *outs) == 0
    assert call() == 0                                         # and the library still works
