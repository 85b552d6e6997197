"""Search engine -- host-side mirror of the hot-path half of the reference's
``ann_solo/spectral_library.py`` (``SpectralLibrary`` :27-500).

What is mirrored (same names, same meaning): the constructor (:46-116: ``SpectralLibrary(
filename)`` over a ``SpectralLibraryReader``, kept as ``_library_reader``),
``_get_hyperparameter_hash`` (:118-131), ``_create_ann_indexes`` (:133-183), ``search`` /
``_search_cascade`` (:193-326), ``_search_batch`` (:328-370), ``_get_library_candidates``
(:372-455), ``_get_ann_index`` (:457-500) and ``shutdown`` (:185-191). What is different by
design: the library is a packed, HBM-resident peak store per precursor charge (built once
through the reader's surface, ``library_store.py``) instead of per-spectrum HDF5 reads, a
whole batch runs through ``asl_search_batch`` in one device pipeline (encode -> IVF top-k ->
precursor post-filter -> shifted-dot best match), and with ``enable_sharding`` every batch of
both cascade levels runs over the ranks of one node (``distributed.py``).

File parsing, FDR/mokapot scoring stay with the reference (out of scope): the
library/query readers and the scorer are injected (defaults: the reference's own
``ann_solo.reader`` when it is importable).
"""
import ctypes as C
import hashlib
import json
import logging
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import faiss_compat as faiss
from .config import Config
from .packed import PackedSpectra
from .spectrum import get_dim, spectra_to_vectors, HASH_SEED
from .spectrum_match import score_flags


@dataclass
class ChargePartition:
    """spec_info['charge'][z] (reader.py:184-191) + the device-resident peak store."""
    charge: int
    ids: np.ndarray                 # library identifiers of the rows
    precursor_mz: np.ndarray        # float32, as the reference stores it
    spectra: PackedSpectra          # device
    handle: C.c_void_p = None       # asl_library_t*
    index: Optional[faiss.Index] = None


@dataclass
class BatchResult:
    """Per-query outputs of one batch (all numpy, length nq)."""
    best_row: np.ndarray            # row inside the charge partition, -1: no candidate
    best_score: np.ndarray
    n_candidates: np.ndarray
    pm_count: np.ndarray
    pm_pairs: np.ndarray            # [nq, stride, 2]
    knn: Optional[np.ndarray] = None

    def peak_matches(self, i) -> np.ndarray:
        return self.pm_pairs[i, :self.pm_count[i]].astype(np.int64)


@dataclass
class TopnBatchResult:
    """Per-query outputs of one top-n batch: the ``n_best`` best library matches of every query,
    best first (score descending, equal scores to the lower library row). Numpy arrays or device
    tensors; ranks beyond a query's candidates hold row -1, score 0.0, count 0."""
    best_row: np.ndarray            # [nq, n_best] rows inside the charge partition
    best_score: np.ndarray          # [nq, n_best] shifted-dot scores
    n_candidates: np.ndarray        # [nq]
    pm_count: np.ndarray            # [nq, n_best]
    pm_pairs: np.ndarray            # [nq, n_best, stride, 2]
    knn: Optional[np.ndarray] = None
    # [nq, 128] int32: the histogram of every query's candidate scores (``score_hist=True``); its rows sum
    # to n_candidates
    score_hist: Optional[np.ndarray] = None

    def peak_matches(self, i, r=0) -> np.ndarray:
        return _to_np(self.pm_pairs[i, r, :int(self.pm_count[i, r])]).astype(np.int64)

    def rank0(self) -> 'BatchResult':
        """The best matches alone, as the single-winner batch returns them (same values)."""
        c = (lambda a: a.contiguous()) if hasattr(self.best_row, 'contiguous') else np.ascontiguousarray
        return BatchResult(c(self.best_row[:, 0]), c(self.best_score[:, 0]), self.n_candidates,
                           c(self.pm_count[:, 0]), c(self.pm_pairs[:, 0]), self.knn)


INDEX_EXT = '.idxmi'      # own container; the reference's FAISS files keep '.idxann' untouched


def _reference_reader_factory(filename: str, config_hash: str):
    """Default library reader: the reference's own ``SpectralLibraryReader`` (reader.py:40-116)
    when the ``ann_solo`` package is installed next to this one."""
    try:
        from ann_solo import reader as ref_reader          # noqa: the reference package
    except Exception as e:                                   # faiss/h5py/... missing
        raise ImportError(
            'SpectralLibrary(filename) needs a library reader: install the reference package '
            '(ann_solo.reader.SpectralLibraryReader) or pass reader_factory=') from e
    return ref_reader.SpectralLibraryReader(filename, config_hash)


def _reference_config():
    """Default options: the reference's parsed ``config`` singleton (``ann_solo.py:76``) when the
    ``ann_solo`` package is installed and ``config.parse()`` has run, else the defaults."""
    try:
        from ann_solo.config import config as ref_config      # noqa: the reference package
    except Exception:
        return None
    return ref_config if getattr(ref_config, '_namespace', None) is not None else None


def _reference_query_reader(filename: str):
    try:
        from ann_solo import reader as ref_reader
    except Exception as e:
        raise ImportError('search(query_filename) needs a query reader: install the reference '
                          'package (ann_solo.reader.read_query_file) or pass query_reader=') from e
    return ref_reader.read_query_file(filename)


class SpectralLibrary:
    _hyperparameters = ['min_mz', 'max_mz', 'bin_size', 'hash_len', 'num_list']

    def __init__(self, library, identifiers=None, config: Config = None,
                 valid: Optional[np.ndarray] = None, index_dir: Optional[str] = None,
                 basename: Optional[str] = None, device='cuda', reader_factory=None,
                 query_reader=None, score_ssms=None, annotation_alignment: str = 'peaks',
                 import_faiss_cache: bool = True):
        """``library`` is one of

        * a file name -- the reference's call, ``SpectralLibrary(filename)``
          (spectral_library.py:46-116): ``reader_factory(filename, hyper_hash)`` (default: the
          reference's ``SpectralLibraryReader``) opens it, the packed store and the ANN indexes
          are cached next to it as ``<library>_<hash7>.spstore`` / ``<library>_<hash7>_<charge>
          .idxmi``; with ``Config.device_library`` a name ending in ``.sptxt`` (any letter case) is read by
          the engine's own reader (``sptxt.read_library``) and ``reader_factory`` is not called;
        * a reader object with the reference reader's surface (``spec_info``,
          ``read_all_spectra()``, optional ``is_recreated`` / ``get_version()`` / ``close()``);
        * a ``PackedSpectra`` of already processed library spectra (``identifiers``: library
          ids, default row numbers; ``valid``: is_valid flags).

        ANN indexes are built for every charge with >= num_list spectra (:100-104) and cached
        under ``index_dir`` when one is known (:98-108). ``query_reader(filename)`` (default: the
        reference's ``read_query_file``) and ``score_ssms(ssms, mode)`` (stands for
        ``utils.score_ssms``, :319-326) serve ``search(query_filename)``.
        ``annotation_alignment='snapshot'`` reproduces the snapshot's use of RAW-peak
        annotations on processed library peaks (reader.py:243-245; see library_store.py).
        ``import_faiss_cache``: with the reference's own index type (``index='ivfflat'``) an
        existing ``<library>_<hash7>_<charge>.idxann`` written by the reference's FAISS is loaded
        (its centroids and list assignments kept) instead of training a new index."""
        self.config = Config.from_reference(config if config is not None
                                            else _reference_config())
        self.device = torch.device(device)
        cfg = self.config
        if cfg.no_gpu:
            # the reference's --no_gpu keeps FAISS on the CPU (spectral_library.py:73-75); this
            # engine IS the GPU path and has no CPU fallback: say so instead of ignoring the flag
            raise _lib.AnnSoloMiError(
                'no_gpu=True: ann_solo_amd is the MI355X path and has no CPU fallback; run the '
                "reference's own SpectralLibrary for a CPU search")
        k_max = _lib.TK_MAX_K
        if cfg.num_probe > k_max:
            # the reference clamps both to 1024 on the GPU (FAISS-GPU's limit, :76-87); this
            # implementation's LDS top-k holds 2048 -- same warning, the larger limit
            logging.warning('Using num_probe=%d (maximum supported value on the GPU), %d was '
                            'supplied', k_max, cfg.num_probe)
        c_max = _lib.TK_MAX_K_PASSES       # beyond k_max the index searches in bounded passes (exact, slower)
        if cfg.num_candidates > c_max:
            logging.warning('Using num_candidates=%d (maximum supported value on the GPU), %d '
                            'was supplied', c_max, cfg.num_candidates)
        self._num_probe = min(cfg.num_probe, k_max)
        self._num_candidates = min(cfg.num_candidates, c_max)
        self._use_gpu = True
        self._ann_filenames: Dict[int, str] = {}
        self._faiss_filenames: Dict[int, str] = {}      # reference caches that can be imported
        self._current_index: Tuple[Optional[int], Optional[faiss.Index]] = (None, None)
        self._query_reader = query_reader or _reference_query_reader
        self._score_ssms = score_ssms
        if cfg.device_fdr and score_ssms is None:       # the engine's own FDR step; an injected callable wins
            from . import fdr
            self._score_ssms = fdr.make_scorer(cfg, self.device)
        self._dist = None
        self._library_reader = None
        self.library_meta: Optional[Dict[int, list]] = None
        self.partitions: Dict[int, ChargePartition] = {}
        verify_file_existence = True
        if isinstance(library, PackedSpectra):
            if cfg.device_decoys:
                raise ValueError('device_decoys needs a library reader or file name: a PackedSpectra holds '
                                 'processed peaks and no peptides')
            self._index_dir = index_dir
            self._basename = basename or 'library'
            self._init_from_packed(library, identifiers, valid)
        else:
            from . import library_store as ls
            own_reader = False
            if isinstance(library, (str, os.PathLike)):
                filename = os.fspath(library)
                own_reader = cfg.device_library and filename.lower().endswith('.sptxt')
                if own_reader and annotation_alignment != 'peaks':
                    raise ValueError(f"annotation_alignment = {annotation_alignment!r} with device_library: the "
                                     "device reader keeps every charge with its peak ('peaks')")
                if not own_reader:
                    self._library_reader = (reader_factory or _reference_reader_factory)(
                        filename, self._get_hyperparameter_hash())
            else:
                self._library_reader = library
                filename = getattr(library, '_filename', None) or cfg.spectral_library_filename
            if cfg.device_decoys and not own_reader:    # decoy row, target row for every spectrum the reader lists
                self._library_reader = ls.DecoyReader(self._library_reader, cfg, self.device)
            if filename:
                stem = os.path.splitext(filename)[0]
                self._index_dir = index_dir if index_dir is not None else (os.path.dirname(stem) or '.')
                self._basename = basename or os.path.basename(stem)
            else:
                self._index_dir, self._basename = index_dir, basename or 'library'
            key = ls.store_hash(cfg, self._get_hyperparameter_hash(), annotation_alignment)
            path = None if self._index_dir is None else os.path.join(
                self._index_dir, f'{self._basename}_{key[:7]}{ls.STORE_EXT}')
            if own_reader:              # the engine's own reader (sptxt.py): no reader_factory, no objects
                from . import sptxt
                self._library_reader = sptxt.read_library(filename, cfg, self.device, path, key)
            if getattr(self._library_reader, 'is_recreated', False):
                logging.warning('ANN indexes were created using non-compatible settings')
                verify_file_existence = False
            if own_reader:
                store = self._library_reader.store
            else:
                store = ls.load_or_build_library_store(self._library_reader, cfg, self.device, path,
                                                       key, annotation_alignment)
            self.library_meta = store.meta
            for z, (a, b) in store.ranges.items():
                rows = torch.arange(a, b)
                info = self._library_reader.spec_info['charge'][z]
                self._add_partition(int(z), store.spectra.select(rows), np.asarray(info['id']),
                                    store.valid[a:b],
                                    np.asarray(info['precursor_mz'], np.float32))
        if cfg.mode == 'ann':
            create = []
            for z in sorted(self.partitions):
                if len(self.partitions[z].ids) < (1 if cfg.index == 'winflat' else cfg.num_list):
                    continue          # infrequent charge: brute force (spectral_library.py:102-104)
                base = f'{self._basename}_{self._get_index_hash()[:7]}'
                self._ann_filenames[z] = os.path.join(self._index_dir or '', f'{base}_{z}{INDEX_EXT}')
                ref = os.path.join(self._index_dir or '', f'{self._basename}_'
                                   f'{self._get_hyperparameter_hash()[:7]}_{z}.idxann')
                if (import_faiss_cache and cfg.index == 'ivfflat' and self._index_dir is not None and
                        verify_file_existence and os.path.isfile(ref) and not cfg.device_decoys):
                    self._faiss_filenames[z] = ref
                if (self._index_dir is None or not verify_file_existence or
                        not (os.path.isfile(self._ann_filenames[z]) or z in self._faiss_filenames)):
                    if self._index_dir is not None:
                        logging.warning('Missing ANN index for charge %d', z)
                    create.append(z)
            if create:
                self._create_ann_indexes(create)
        if cfg.num_gpus and cfg.num_gpus > 1:      # additive flag --num_gpus (config.py)
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_initialized() else 1
            if world != cfg.num_gpus:
                raise RuntimeError(
                    f'num_gpus={cfg.num_gpus} needs a torch.distributed job of that many ranks '
                    f'(one process per GPU, e.g. torchrun --nproc-per-node {cfg.num_gpus}); '
                    f'this process sees {world}')
            self.enable_sharding()

    def _init_from_packed(self, library: PackedSpectra, identifiers, valid) -> None:
        n = library.n
        ids = np.arange(n) if identifiers is None else np.asarray(identifiers)
        pz = library.precursor_charge.cpu().numpy()
        valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        for z in np.unique(pz):
            rows = np.nonzero(pz == z)[0]
            self._add_partition(int(z), library.select(torch.as_tensor(rows)), ids[rows],
                                valid[rows], None)

    def _add_partition(self, z: int, spectra: PackedSpectra, ids, valid, pmz32) -> None:
        part = spectra.to(self.device).contiguous()
        if pmz32 is None:       # spec_info stores the precursor m/z column as float32 (reader.py:186-189)
            pmz32 = part.precursor_mz.cpu().numpy().astype(np.float32)
        pmz32 = np.ascontiguousarray(pmz32, np.float32)
        v = np.ascontiguousarray(np.asarray(valid).astype(np.uint8))
        h = _lib.lib().asl_library_create(C.byref(_lib.peaks_struct(part)), _lib.ptr(pmz32),
                                          _lib.ptr(v))
        if not h:
            _lib.check(-1)
        self.partitions[z] = ChargePartition(z, np.asarray(ids), pmz32, part, C.c_void_p(h))

    # ------------------------------------------------------------------ reference mirrors
    def _get_hyperparameter_hash(self) -> str:
        b = json.dumps({hp: self.config[hp] for hp in self._hyperparameters}).encode('utf-8')
        return hashlib.sha1(b).hexdigest()

    def _get_index_hash(self) -> str:
        """Hash in the cached index file names: the reference's five hyper-parameters for its
        own configuration (IVF-Flat, FAISS' default 25 iterations and seed 1234 -- same 7 hex
        digits as the reference's ``.idxann`` name); any additive option of this implementation
        (index kind, PQ shape, trainer settings) is hashed in as well, so switching it can never
        pick up a stale file."""
        cfg = self.config
        if (cfg.index == 'ivfflat' and cfg.kmeans_niter == 25 and cfg.seed == 1234 and
                cfg.flat_storage == 'fp32' and not cfg.device_decoys):
            return self._get_hyperparameter_hash()
        d = {hp: cfg[hp] for hp in self._hyperparameters}
        d.update(index=cfg.index, kmeans_niter=cfg.kmeans_niter, seed=cfg.seed)
        if cfg.device_decoys:           # the index then holds the decoy rows too
            from .library_store import decoy_options
            d.update(decoys=decoy_options(cfg))
        if cfg.index in ('ivfflat', 'winflat') and cfg.flat_storage != 'fp32':
            d.update(flat_storage=cfg.flat_storage)
        if cfg.index == 'ivfpq':
            d.update(pq_m=cfg.pq_m, pq_bits=cfg.pq_bits)
            if cfg.refine_k:
                d.update(refine_k=cfg.refine_k)
            if not cfg.pq_by_residual:      # (on: every file name as before the option existed)
                d.update(pq_by_residual=False)
        return hashlib.sha1(json.dumps(d).encode('utf-8')).hexdigest()

    def _encode(self, spectra: PackedSpectra) -> torch.Tensor:
        cfg = self.config
        out = torch.empty((spectra.n, cfg.hash_len), dtype=torch.float32, device=self.device)
        spectra_to_vectors(spectra.mz, spectra.intensity, spectra.offsets, cfg.min_mz, cfg.max_mz,
                           cfg.bin_size, cfg.hash_len, True, out)
        return out

    def _create_ann_indexes(self, charges: List[int]) -> None:
        cfg = self.config
        for z in charges:
            part = self.partitions[z]
            vectors = self._encode(part.spectra)
            if cfg.index == 'winflat':      # the vectors as given: nothing to train
                ann_index = faiss.IndexWindowFlat(cfg.hash_len, storage=cfg.flat_storage)
                ann_index.add(vectors)
                if self._index_dir is not None:
                    faiss.write_index(ann_index, self._ann_filenames[z])
                part.index = ann_index
                del vectors
                continue
            quantizer = faiss.IndexFlatIP(cfg.hash_len)
            if cfg.index == 'ivfpq':
                ann_index = faiss.IndexIVFPQ(quantizer, cfg.hash_len, cfg.num_list, cfg.pq_m,
                                             cfg.pq_bits, faiss.METRIC_INNER_PRODUCT)
            else:
                ann_index = faiss.IndexIVFFlat(quantizer, cfg.hash_len, cfg.num_list,
                                               faiss.METRIC_INNER_PRODUCT, storage=cfg.flat_storage)
            ann_index.seed = cfg.seed
            ann_index.set_niter(cfg.kmeans_niter)
            if cfg.index == 'ivfpq' and cfg.refine_k:
                ann_index.set_refine(cfg.refine_k)
            if cfg.index == 'ivfpq' and not cfg.pq_by_residual:
                ann_index.by_residual = False
            ann_index.train(vectors)
            ann_index.add(vectors)
            if self._index_dir is not None:
                faiss.write_index(ann_index, self._ann_filenames[z])
            part.index = ann_index
            del vectors

    def _index_matches(self, idx: faiss.Index, part: ChargePartition) -> bool:
        cfg, i = self.config, idx.info()
        kind = {'ivfpq': 2, 'winflat': 3}.get(cfg.index, 1)
        if kind == 3:       # one list: num_list plays no part
            return (i.kind == 3 and i.d == cfg.hash_len and i.ntotal == len(part.ids) and i.shard_world == 1 and
                    idx.storage == cfg.flat_storage)
        return (i.kind == kind and i.d == cfg.hash_len and i.nlist == cfg.num_list and
                i.ntotal == len(part.ids) and bool(i.trained) and i.shard_world == 1 and
                (kind != 2 or (i.pq_m == cfg.pq_m and i.pq_ksub == (1 << cfg.pq_bits) and
                               idx.by_residual == bool(cfg.pq_by_residual))) and
                (kind != 1 or idx.storage == cfg.flat_storage))

    def _get_ann_index(self, charge: int) -> faiss.Index:
        part = self.partitions[charge]
        if part.index is None:
            idx = None
            imported = False
            if not os.path.isfile(self._ann_filenames[charge]) and charge in self._faiss_filenames:
                try:        # the reference's FAISS cache: its centroids, its list assignments
                    idx = faiss.read_index_faiss(self._faiss_filenames[charge],
                                                 storage=self.config.flat_storage)
                    imported = True
                    logging.info('Imported the FAISS index %s', self._faiss_filenames[charge])
                except (ValueError, OSError, _lib.AnnSoloMiError) as e:
                    logging.warning('FAISS index %s not usable (%s): building a new index',
                                    self._faiss_filenames[charge], e)
            else:
                try:
                    idx = faiss.read_index(self._ann_filenames[charge])
                except _lib.AnnSoloMiError as e:
                    logging.warning('ANN index %s unreadable (%s): rebuilding',
                                    self._ann_filenames[charge], e)
            if idx is not None and not self._index_matches(idx, part):
                # e.g. another library under the same base name: out-of-range ids would be
                # dropped silently by the rescoring bounds check -- never search a stale index
                logging.warning('ANN index %s does not match the library/configuration: '
                                'rebuilding', self._ann_filenames[charge])
                idx = None
            if idx is None:
                self._create_ann_indexes([charge])
            else:
                part.index = idx
                if imported and self._index_dir is not None:     # next time: our own container
                    faiss.write_index(idx, self._ann_filenames[charge])
            d = self._dist
            if d is not None and d.world > 1:
                part.index.shard(d.rank, d.world)
        part.index.nprobe = self._num_probe
        part.index.set_window_scan(self.config.ann_window == 'pre')     # per index handle
        self._current_index = charge, part.index
        return part.index

    # ------------------------------------------------------------------ multi-GPU
    def enable_sharding(self, group=None) -> None:
        """List-shard every ANN index over the ranks of ``group`` (default: all ranks of the
        initialised ``torch.distributed`` job) -- SURVEY.md 8(e). From here on every batch of
        both cascade levels runs on all ranks (``distributed.sharded_cascade_batch``): the open
        search scans this rank's inverted lists for the whole batch and exchanges per-shard
        top-k, the standard search is data-parallel over the queries; every rank ends up with
        the results of the whole batch. Every rank must call ``search`` with the same queries."""
        if self.config.ann_window == 'pre':
            raise ValueError("enable_sharding: ann_window = 'pre' does not run on a sharded index")
        if self.config.index == 'winflat':
            raise ValueError("enable_sharding: index = 'winflat' has one list and is not sharded")
        if getattr(self, '_search_subset', False):
            raise ValueError('enable_sharding: a search subset (set_search_subset) does not run on a sharded library')
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        if world > 1 and self.config.device_fdr:
            # (a level's SSMs are gathered on rank 0 only after its gate: every rank would train on its own)
            raise ValueError('enable_sharding: device_fdr does not run on a sharded index')
        if world > 1 and self.config.chimeric_search:
            raise ValueError('enable_sharding: chimeric_search does not run on a sharded index')
        if self._dist is not None and self._dist.world > 1:
            raise RuntimeError('enable_sharding: the indexes are sharded already')
        self._dist = SimpleNamespace(group=group, world=world, rank=rank, backends={})
        if world > 1:
            for part in self.partitions.values():
                if part.index is not None:
                    part.index.shard(rank, world)

    def set_pipeline(self, on=True) -> None:
        """Two-stream software pipeline of the device hot path (``asl_set_pipeline``): with
        ``device_out=True`` an open-search ``_search_batch`` returns without waiting, and the
        encoder + coarse quantiser of the next batch run under the list scan of this one.
        Results are valid after ``synchronize()``; values are bit-identical either way."""
        self.synchronize()
        _lib.check(_lib.lib().asl_set_pipeline(int(on)))       # True/1: two streams, 3: three
        self._pipeline_on = bool(on)

    def synchronize(self) -> None:
        """Wait for the batches in flight; their inputs and outputs may be released afterwards."""
        try:
            _lib.check(_lib.lib().asl_synchronize())
        finally:
            getattr(self, '_inflight', []).clear()

    def _hold(self, *tensors) -> None:
        """Pipeline mode returns before the device has read the inputs or written the outputs,
        on streams PyTorch's allocator knows nothing about: a tensor released by the caller could be
        handed out again (and overwritten) while a kernel still uses it. Every array of a pipelined
        call is therefore kept alive here until the next synchronisation."""
        if not hasattr(self, '_inflight'):
            self._inflight = []
        self._inflight.append(tensors)
        if len(self._inflight) >= 32:      # bound what is pinned: waiting here is cheap
            self.synchronize()

    def _shard_backend(self, charge: int, mode: str):
        from .distributed import HipShardBackend
        key = (charge, mode)
        if key not in self._dist.backends:
            self._dist.backends[key] = HipShardBackend(self, charge, mode)
        return self._dist.backends[key]

    def shutdown(self) -> None:
        if getattr(self, '_inflight', None):
            self.synchronize()
        reader = getattr(self, '_library_reader', None)
        if reader is not None and hasattr(reader, 'close'):
            reader.close()                       # spectral_library.py:189
        for part in self.partitions.values():
            if part.handle:
                _lib.lib().asl_library_free(part.handle)
                part.handle = None
            part.index = None

    def _tolerance(self, mode: str):
        cfg = self.config
        if mode == 'std':
            return cfg.precursor_tolerance_mass, cfg.precursor_tolerance_mode
        if mode == 'open':
            return cfg.precursor_tolerance_mass_open, cfg.precursor_tolerance_mode_open
        raise ValueError('Unknown search mode')

    def _uses_ann(self, charge: int, mode: str) -> bool:
        return self.config.mode == 'ann' and mode == 'open' and charge in self._ann_filenames

    def _search_batch(self, queries: PackedSpectra, charge: int, mode: str,
                      want_knn: bool = False, device_out: bool = False, windows=None,
                      shifts: Optional[bool] = None) -> Optional[BatchResult]:
        """One batch of same-charge, processed query spectra (spectral_library.py:328-370):
        through the device hot path of this GPU, or -- after ``enable_sharding`` on more than
        one rank -- over all ranks. Returns None when the library has no spectra of that charge
        (:411-412). ``windows``: None, or one closed interval (lo, hi) of library precursor m/z per query
        ([nq, 2] float64, numpy or a device tensor) -- the candidates are then the rows whose float32
        precursor m/z lies inside it (``ASL_TOL_INTERVAL``), whatever the level's tolerance is; scores
        still use the query's own precursor m/z. ``shifts``: None, or whether the dot product shifts peaks,
        whatever ``Config.allow_peak_shifts`` says (the chimeric level: False). One GPU, both."""
        d = getattr(self, '_dist', None)
        if d is None or d.world == 1:
            if shifts is not None:
                return self._search_batch_local(queries, charge, mode, want_knn, device_out, windows=windows,
                                                shifts=shifts)
            if windows is None:     # (engines that override _search_batch_local with its older signature)
                return self._search_batch_local(queries, charge, mode, want_knn, device_out)
            return self._search_batch_local(queries, charge, mode, want_knn, device_out, windows=windows)
        if windows is not None or shifts is not None:
            raise ValueError('windows= / shifts= do not run on a sharded index')
        tol_val, tol_mode = self._tolerance(mode)
        if tol_mode not in ('Da', 'ppm'):
            raise ValueError('Unknown precursor tolerance mode')
        if charge not in self.partitions or queries.n == 0:
            return None if charge not in self.partitions else self._search_batch_local(
                queries, charge, mode)
        from .distributed import sharded_cascade_batch
        return sharded_cascade_batch(self._shard_backend(charge, mode), queries, mode,
                                     self._uses_ann(charge, mode), d.group)

    def _search_batch_local(self, queries: PackedSpectra, charge: int, mode: str,
                            want_knn: bool = False, device_out: bool = False,
                            pm_stride: Optional[int] = None, windows=None,
                            shifts: Optional[bool] = None) -> Optional[BatchResult]:
        """One batch on this GPU alone (the index must not be sharded for open searches)."""
        tol_val, tol_mode = self._tolerance(mode)
        if tol_mode not in ('Da', 'ppm'):
            raise ValueError('Unknown precursor tolerance mode')
        if charge not in self.partitions:
            return None
        cfg = self.config
        part = self.partitions[charge]
        use_ann = self._uses_ann(charge, mode)
        idx = self._get_ann_index(charge) if use_ann else None
        q = queries.to(self.device).contiguous()
        nq = q.n
        k = self._num_candidates
        stride = pm_stride or q.max_peaks()
        xp = torch if device_out else np
        kw = dict(device=self.device) if device_out else {}
        mk = (lambda shape, dt: torch.empty(shape, dtype=dt, **kw)) if device_out else \
             (lambda shape, dt: np.empty(shape, dt))
        best_row = mk((nq,), xp.int32)
        best_score = mk((nq,), xp.float64)
        n_cand = mk((nq,), xp.int32)
        pm_count = mk((nq,), xp.int32)
        # (the kernel writes every slot: matches first, zeros beyond pm_count)
        pm_pairs = (torch.empty((nq, stride, 2), dtype=torch.int32, **kw) if device_out
                    else np.empty((nq, stride, 2), np.uint32))
        knn = mk((nq, k), xp.int64) if (want_knn and use_ann) else None
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, k, self._num_probe, charge,
                                 float(tol_val), 0 if tol_mode == 'Da' else 1,
                                 cfg.fragment_mz_tolerance,
                                 score_flags(cfg.allow_peak_shifts if shifts is None else shifts,
                                             cfg.fragment_tolerance_unit),
                                 int(use_ann))
        windows = self._interval_windows(P, windows, nq)
        _lib.check(_lib.lib().asl_search_batch(
            part.handle, idx._h if idx is not None else None, C.byref(_lib.peaks_struct(q)),
            C.byref(P), _lib.ptr(best_row), _lib.ptr(best_score), _lib.ptr(n_cand),
            _lib.ptr(pm_count), _lib.ptr(pm_pairs), stride, _lib.ptr(knn)))
        if device_out and use_ann and getattr(self, '_pipeline_on', False):
            self._hold(q, best_row, best_score, n_cand, pm_count, pm_pairs, knn, windows)
        return BatchResult(best_row, best_score, n_cand, pm_count, pm_pairs, knn)

    def _interval_windows(self, P, windows, nq: int):
        """``windows=`` of a search call into its parameter block: [nq, 2] float64 on the device,
        ``precursor_mode`` 2 (``ASL_TOL_INTERVAL``). Returns the tensor (the caller keeps it alive)."""
        if windows is None:
            return None
        if not hasattr(windows, 'data_ptr'):
            windows = torch.from_numpy(np.ascontiguousarray(windows, np.float64))
        windows = windows.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(windows.shape) != (nq, 2):
            raise ValueError(f'windows: {tuple(windows.shape)} for {nq} queries; one interval (lo, hi) per query')
        P.precursor_mode = faiss.TOL_MODES['interval']
        P.precursor_window = _lib.ptr(windows)
        return windows

    def set_match_groups(self, groups: Optional[Dict[int, np.ndarray]]) -> None:
        """Group ids of the library rows for distinct ranked matches: ``{charge: int32 array}``, one
        id per row of that charge partition (e.g. its peptide; negative: ungrouped), copied to the
        partition's device handle (``asl_library_set_groups``). Every partition must be named;
        ``None`` drops the columns again."""
        L = _lib.lib()
        self._match_groups_from = None
        if groups is None:
            for part in self.partitions.values():
                _lib.check(L.asl_library_set_groups(part.handle, 0, None))
            return
        missing = sorted(set(self.partitions) - set(groups))
        if missing:
            raise ValueError(f'set_match_groups: no group ids for charge(s) {missing}')
        for z, part in self.partitions.items():
            g = groups[z]
            if isinstance(g, (list, tuple, np.ndarray)):
                g = np.ascontiguousarray(g, np.int32)
            _lib.check(L.asl_library_set_groups(part.handle, len(g), _lib.ptr(g)))

    def set_search_subset(self, subset: Optional[Dict[int, np.ndarray]]) -> None:
        """Search a subset of the library: ``{charge: bool array}``, one flag per row of that charge
        partition (True: selected), copied to the partition's device handle
        (``asl_library_set_selection``). Every partition must be named; ``None`` drops the subset.
        Both cascade levels honour it: the standard search walks the selected rows of the window, the
        open search's scan chooses its ``num_candidates`` among the selected vectors of the probed
        lists (never a filter behind the top-k), and results are what a library of the selected rows
        alone -- same row numbers, same index lists -- would return. Does not run on a sharded library."""
        d = getattr(self, '_dist', None)
        if d is not None and d.world > 1:
            raise ValueError('set_search_subset does not run on a sharded library')
        if subset is None:
            L = _lib.lib()
            for part in self.partitions.values():
                if part.handle is not None:
                    _lib.check(L.asl_library_set_selection(part.handle, 0, None))
            self._search_subset = False
            return
        missing = sorted(set(self.partitions) - set(subset))
        if missing:
            raise ValueError(f'set_search_subset: no flags for charge(s) {missing}')
        keep = {}
        for z, part in self.partitions.items():
            k = subset[z]
            if isinstance(k, (list, tuple, np.ndarray)):
                k = np.ascontiguousarray(np.asarray(k).astype(bool), np.uint8)
            else:                                   # a torch tensor, host or device
                k = (k != 0).to(dtype=torch.uint8).contiguous()
            if tuple(k.shape) != (len(part.ids),):
                raise ValueError(f'set_search_subset: {tuple(k.shape)} flags for the {len(part.ids)} rows of '
                                 f'charge {z}')
            keep[z] = k
        L = _lib.lib()
        for z, part in self.partitions.items():
            _lib.check(L.asl_library_set_selection(part.handle, len(part.ids), _lib.ptr(keep[z])))
        self._search_subset = True

    def _match_groups_from_peptides(self, library_meta) -> None:
        """``distinct_matches``: the group of a library row is its peptide (``library_meta[charge]
        [row]['peptide']``) -- equal strings share an id, ``None`` is ungrouped (-1); ids are
        assigned per charge partition. Done once per metadata object."""
        if getattr(self, '_match_groups_from', None) is library_meta:
            return
        groups = {}
        for z, part in self.partitions.items():
            cont, n = library_meta[z], len(part.ids)
            if hasattr(cont, 'column'):
                pep = list(cont.column('peptide', np.arange(n)))
            else:
                pep = [cont[i].get('peptide') for i in range(n)]
            ids: Dict = {}
            groups[z] = np.fromiter((-1 if p is None else ids.setdefault(p, len(ids)) for p in pep),
                                    np.int32, n)
        self.set_match_groups(groups)
        self._match_groups_from = library_meta

    def search_batch_topn(self, queries: PackedSpectra, charge: int, mode: str, n_best: int,
                          want_knn: bool = False, device_out: bool = False,
                          pm_stride: Optional[int] = None, distinct: bool = False,
                          windows=None, score_hist: bool = False,
                          shifts: Optional[bool] = None) -> Optional[TopnBatchResult]:
        """``_search_batch_local`` for the ``n_best`` (1 .. 16) best library matches of every query
        (``asl_search_batch_topn``): every cascade level and index mode, on this GPU alone.
        Synchronous -- the call never joins the two-stream pipeline. Rank 0 (and ``n_candidates``,
        ``knn``) is what ``_search_batch_local`` returns, bit for bit. ``distinct``: one rank per
        group of ``set_match_groups`` (``asl_search_batch_topn_distinct``; an error without groups).
        ``windows``, ``shifts``: as in ``_search_batch``. ``score_hist``: the result also carries the histogram of
        every query's candidate scores, ``[nq, 128]`` int32 (``asl_search_batch_topn_hist``; 128 bins of
        width 1/128, ``score_stats.bin_of``), whose rows sum to ``n_candidates``; nothing else changes."""
        d = getattr(self, '_dist', None)
        if d is not None and d.world > 1:
            raise ValueError('search_batch_topn does not run on a sharded index')
        tol_val, tol_mode = self._tolerance(mode)
        if tol_mode not in ('Da', 'ppm'):
            raise ValueError('Unknown precursor tolerance mode')
        if charge not in self.partitions:
            return None
        cfg = self.config
        part = self.partitions[charge]
        use_ann = self._uses_ann(charge, mode)
        idx = self._get_ann_index(charge) if use_ann else None
        q = queries.to(self.device).contiguous()
        nq, n = q.n, int(n_best)
        k = self._num_candidates
        stride = pm_stride or q.max_peaks()
        xp = torch if device_out else np
        mk = (lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)) if device_out else \
             (lambda shape, dt: np.empty(shape, dt))
        shape = (nq, max(n, 0))
        best_row = mk(shape, xp.int32)
        best_score = mk(shape, xp.float64)
        n_cand = mk((nq,), xp.int32)
        pm_count = mk(shape, xp.int32)
        pm_pairs = mk(shape + (stride, 2), torch.int32 if device_out else np.uint32)
        knn = mk((nq, k), xp.int64) if (want_knn and use_ann) else None
        _, min_bound, _ = get_dim(cfg.min_mz, cfg.max_mz, cfg.bin_size)
        P = _lib.AslSearchParams(min_bound, cfg.bin_size, HASH_SEED, k, self._num_probe, charge,
                                 float(tol_val), 0 if tol_mode == 'Da' else 1,
                                 cfg.fragment_mz_tolerance,
                                 score_flags(cfg.allow_peak_shifts if shifts is None else shifts,
                                             cfg.fragment_tolerance_unit),
                                 int(use_ann))
        windows = self._interval_windows(P, windows, nq)
        if score_hist:
            hist = mk((nq, _lib.SCORE_HIST_BINS), xp.int32)
            _lib.check(_lib.lib().asl_search_batch_topn_hist(
                part.handle, idx._h if idx is not None else None, C.byref(_lib.peaks_struct(q)),
                C.byref(P), n, int(bool(distinct)), _lib.ptr(best_row), _lib.ptr(best_score), _lib.ptr(n_cand),
                _lib.ptr(pm_count), _lib.ptr(pm_pairs), stride, _lib.ptr(knn), _lib.ptr(hist)))
            return TopnBatchResult(best_row, best_score, n_cand, pm_count, pm_pairs, knn, hist)
        call = _lib.lib().asl_search_batch_topn_distinct if distinct else _lib.lib().asl_search_batch_topn
        _lib.check(call(
            part.handle, idx._h if idx is not None else None, C.byref(_lib.peaks_struct(q)),
            C.byref(P), n, _lib.ptr(best_row), _lib.ptr(best_score), _lib.ptr(n_cand),
            _lib.ptr(pm_count), _lib.ptr(pm_pairs), stride, _lib.ptr(knn)))
        return TopnBatchResult(best_row, best_score, n_cand, pm_count, pm_pairs, knn)

    def _get_library_candidates(self, queries: PackedSpectra, charge: int, mode: str, windows=None):
        """CSR candidate lists (library rows of the charge partition, ascending) after the
        precursor filter -- and, in open+ann mode, after the ANN filter. Diagnostic
        mirror of spectral_library.py:372-455; ``_search_batch`` never materialises it.
        ``windows``: as in ``_search_batch`` (the precursor filter is then the interval test)."""
        tol_val, tol_mode = self._tolerance(mode)
        if charge not in self.partitions:
            return None
        part = self.partitions[charge]
        nq = queries.n
        qp = np.ascontiguousarray(queries.precursor_mz.cpu().numpy(), np.float64)
        tol_code = 0 if tol_mode == 'Da' else 1
        if windows is not None:
            qp = np.ascontiguousarray(_to_np(windows), np.float64)
            if qp.shape != (nq, 2):
                raise ValueError(f'windows: {qp.shape} for {nq} queries; one interval (lo, hi) per query')
            tol_code = faiss.TOL_MODES['interval']
        off = np.empty(nq + 1, np.int32)
        _lib.check(_lib.lib().asl_window_candidates(part.handle, nq, _lib.ptr(qp), charge,
                                                    float(tol_val), tol_code,
                                                    _lib.ptr(off), None))
        rows = np.empty(int(off[-1]), np.int64)
        _lib.check(_lib.lib().asl_window_candidates(part.handle, nq, _lib.ptr(qp), charge,
                                                    float(tol_val), tol_code,
                                                    _lib.ptr(off), _lib.ptr(rows)))
        lists = [rows[off[i]:off[i + 1]] for i in range(nq)]
        if self.config.mode == 'ann' and mode == 'open' and charge in self._ann_filenames:
            if self.config.index == 'winflat':      # the k best vectors OF the window: the fused call's neighbour rows
                I = _to_np(self._search_batch(queries, charge, mode, want_knn=True, windows=windows).knn)
                return [np.sort(I[i][I[i] >= 0]) for i in range(nq)]
            idx = self._get_ann_index(charge)
            _, I = idx.search(self._encode(queries.to(self.device)), self._num_candidates)
            I = I.cpu().numpy()
            lists = [np.intersect1d(l, I[i][I[i] >= 0]) for i, l in enumerate(lists)]
        return lists

    def candidate_rank(self, queries: PackedSpectra, charge: int, rows, nprobe: Optional[int] = None,
                       window: bool = False):
        """Where library row ``rows[i]`` of the charge partition stands in the ANN index's neighbour
        order for query i (``faiss_compat.Index.rank_of``): ``(rank, score, scope)`` as numpy arrays.
        The query is retrieved by the open search for every ``num_candidates > rank`` and for no
        smaller one; -1: it never is (its list is not probed, or -- ``window=True`` -- it fails the
        open-level precursor window). ``nprobe``: None = the configured ``num_probe``, 0 = every list.
        ``window=False`` ranks over the probed lists as the post-filter search does (``ann_window =
        'post'``: the needed k); ``window=True`` over their in-window vectors only (``'pre'``), with
        the partition's precursor column as the key. This is the measurement the reference's
        notebooks/iprg2012_num_candidates.ipynb makes with ``num_neighbors = 1000000``."""
        if charge not in self.partitions:
            return None
        if getattr(self, '_dist', None) is not None and self._dist.world > 1:
            raise ValueError('candidate_rank: does not run on a sharded index')
        if self.config.index == 'winflat':
            raise ValueError("candidate_rank: index = 'winflat' has no neighbour order over probed lists to rank in")
        part = self.partitions[charge]
        idx = self._get_ann_index(charge)
        q = queries.to(self.device).contiguous()
        rows = torch.as_tensor(np.asarray(rows, np.int64), device=self.device)
        win = None
        if window:
            tol_val, tol_mode = self._tolerance('open')
            if tol_mode not in ('Da', 'ppm'):
                raise ValueError('Unknown precursor tolerance mode')
            win = (torch.as_tensor(part.precursor_mz, device=self.device), q.precursor_mz.double(), charge,
                   float(tol_val), tol_mode)
        rank, score, scope = idx.rank_of(self._encode(q), rows, self._num_probe if nprobe is None else nprobe, win)
        return rank.cpu().numpy(), score.cpu().numpy(), scope.cpu().numpy()

    def search_charge_batches(self, query_spectra: Dict[int, PackedSpectra], mode: str
                              ) -> Iterator[Tuple[int, int, int, np.ndarray, float]]:
        """One cascade level over per-charge query sets, batched like
        ``_search_cascade`` (:301-317). Yields ``(charge, query_index_in_set, library_id,
        peak_matches[n,2], score)`` for every query with at least one candidate."""
        bs = self.config.batch_size
        for charge, qs in query_spectra.items():
            for b0 in range(0, qs.n, bs):
                rows = torch.arange(b0, min(b0 + bs, qs.n))
                res = self._search_batch(qs.select(rows), charge, mode)
                if res is None:
                    continue
                part = self.partitions[charge]
                for i in range(len(rows)):
                    if res.best_row[i] >= 0:
                        yield (charge, b0 + i, part.ids[res.best_row[i]], res.peak_matches(i),
                               float(res.best_score[i]))

    # ------------------------------------------------------------------ cascade driver
    def search(self, query, query_meta: Optional[Dict[int, list]] = None,
               library_meta: Optional[Dict[int, list]] = None, score_ssms=None) -> list:
        """``SpectralLibrary.search(query_filename)`` (spectral_library.py:193-262): identify all
        spectra of a query file. ``query`` is a file name (read by the injected ``query_reader``,
        default the reference's ``read_query_file``), an iterable of query spectrum objects
        (``identifier, precursor_mz, precursor_charge`` -- None: tried at 2 and 3, :213-223 --
        ``mz, intensity``, optional ``retention_time, index``), or the packed form of
        ``search_packed``. Queries are preprocessed in batches on the device, low-quality ones
        dropped (:225-228). With ``Config.device_mgf`` a file name ending in ``.mgf`` (any letter case)
        is read by ``mgf.read_mgf_packed`` -- parsed on the device, the same packed queries -- instead of
        ``query_reader`` and ``pack_queries``; with ``Config.device_mzml`` a name ending in ``.mzml`` is read by
        ``mzml.read_mzml_packed`` in the same way, and with ``Config.device_mzxml`` a name ending in ``.mzxml`` by
        ``mzxml.read_mzxml_packed``. Returns the identifications as SSM records with the attributes
        ``writer.write_mztab`` consumes (writer.py:129-148)."""
        if isinstance(query, dict):
            return self.search_packed(query, query_meta, library_meta, score_ssms)
        from .library_store import pack_queries
        if (self.config.device_mgf and isinstance(query, (str, os.PathLike)) and
                os.fspath(query).lower().endswith('.mgf')):
            # the engine's own reader: parsed by kernels, no query_reader, no pack_queries (mgf.py)
            from .mgf import read_mgf_packed
            logging.info('Process file %s', query)
            query_spectra, qmeta = read_mgf_packed(os.fspath(query), self.config, self.device)
        elif (self.config.device_mzml and isinstance(query, (str, os.PathLike)) and
                os.fspath(query).lower().endswith('.mzml')):
            # tags parsed and arrays decoded by kernels (mzml.py)
            from .mzml import read_mzml_packed
            logging.info('Process file %s', query)
            query_spectra, qmeta = read_mzml_packed(os.fspath(query), self.config, self.device)
        elif (self.config.device_mzxml and isinstance(query, (str, os.PathLike)) and
                os.fspath(query).lower().endswith('.mzxml')):
            # nested scans parsed and their streams decoded by kernels (mzxml.py)
            from .mzxml import read_mzxml_packed
            logging.info('Process file %s', query)
            query_spectra, qmeta = read_mzxml_packed(os.fspath(query), self.config, self.device)
        else:
            if isinstance(query, (str, os.PathLike)):
                logging.info('Process file %s', query)
                query = self._query_reader(os.fspath(query))
            query_spectra, qmeta = pack_queries(query, self.config, self.device)
        lmeta = library_meta if library_meta is not None else self.library_meta
        if lmeta is None:
            raise ValueError('search(): no library metadata (library built from a PackedSpectra); '
                             'pass library_meta=')
        return self.search_packed(query_spectra, qmeta, lmeta,
                                  score_ssms or getattr(self, '_score_ssms', None))

    def search_packed(self, query_spectra: Dict[int, PackedSpectra], query_meta: Dict[int, list],
                      library_meta: Dict[int, list], score_ssms=None) -> 'SSMTable':
        """``SpectralLibrary.search`` (spectral_library.py:193-262) over packed, already
        processed query spectra split by precursor charge (the file parsing and
        ``process_spectrum`` filtering of :207-228 happen before; queries of unknown charge
        are entered once per candidate charge with the same identifier; inside one charge set
        identifiers are unique).

        ``query_meta[charge][i]`` / ``library_meta[charge][row]``: mappings with the reference's
        attribute names (see ``spectrum.ssms_from_batch``). A query record may also carry
        ``isolation_window = (lo, hi)``, the m/z interval its precursor is known to lie in (wide-window
        DDA, DIA pseudo-spectra; lo <= hi, else ``ValueError``): when EVERY query of a charge has one, the
        open level takes its candidates from the library rows whose precursor m/z lies inside that
        interval, instead of the window around ``precursor_mz`` (``precursor_tolerance_mass_open`` or
        ``Config.precursor_window_open``); scores still use ``precursor_mz``. One GPU: ``ValueError`` on
        a sharded library. ``score_ssms`` stands for
        ``utils.score_ssms`` (:319-326, mokapot -- out of scope): called as ``score_ssms(ssms,
        mode)`` with a list of SSM records it assigns ``search_engine_score`` / ``q`` and
        returns the SSMs to keep; a callable with the attribute ``columnar = True`` receives the
        ``SSMTable`` itself instead, writes ``table.q`` (and ``table.score``) and may return a
        keep-mask -- no per-SSM Python objects on the search path; one with ``uses_features = True``
        also finds the batches' 33 similarity columns in ``table.features``. Default: with
        ``Config.device_fdr`` the engine's own scorer (fdr.py: ``CosineTDC``, ``PercolatorTDC`` or, with
        ``Config.device_forest``, ``ForestTDC`` by ``Config.model``), else cosine as the score, q = 0 (everything accepted).

        With ``Config.chimeric_search`` one more level follows the last one (``_chimeric_level``): the peaks
        every accepted identification explains are taken out of its query and the residue is searched again
        inside the query's isolation window; what it finds is appended with ``chimeric_rank`` 1. The table may
        then hold TWO SSMs for one query identifier (mzTab allows several PSMs per spectrum).

        Returns the identifications (one per query identifier) as an ``SSMTable``: a sequence
        of SSM records materialised on access (``len``, iteration, indexing), ready for
        ``writer.write_mztab``; its columns (``charge, qrow, lib_row, score, q``) are there for
        consumers that do not want 10^5 Python objects."""
        cfg = self.config
        if cfg.distinct_matches and int(cfg.num_matches) > 1:
            self._match_groups_from_peptides(library_meta)
        score_ssms = score_ssms or getattr(self, '_score_ssms', None)
        do_cascade_open = (cfg.precursor_tolerance_mass_open is not None and
                           cfg.precursor_tolerance_mode_open is not None)
        uid = _query_uids(query_meta, list(query_spectra))
        remaining = {z: np.arange(q.n, dtype=np.int64) for z, q in query_spectra.items()}
        # cascade level 1: standard search (:238-245); with a second level only the confident
        # identifications are retained
        t1 = self._search_cascade(query_spectra, query_meta, library_meta, remaining, 'std',
                                  score_ssms, uid)
        n_identified = int((t1.q < cfg.fdr).sum())
        # (message parsed by the reference's notebooks: kept verbatim, spectral_library.py:243)
        logging.info('%d spectra identified after the standard search', n_identified)
        if not do_cascade_open:
            if cfg.chimeric_search:
                t1 = self._chimeric_level(t1, query_spectra, query_meta, library_meta, score_ssms, uid, n_identified)
            return t1
        t1 = t1.take(t1.q < cfg.fdr)
        # cascade level 2: open search on the queries not identified so far (:249-259)
        if uid is None:
            for z in remaining:
                done = np.zeros(len(remaining[z]), bool)
                done[t1.qrow[t1.charge == z]] = True
                remaining[z] = remaining[z][~done]
        else:
            found = t1.uids(uid)
            remaining = {z: rows[~np.isin(uid[z][rows], found)] for z, rows in remaining.items()}
        t2 = self._search_cascade(query_spectra, query_meta, library_meta, remaining, 'open',
                                  score_ssms, uid)
        n_identified += int((t2.q < cfg.fdr).sum())
        logging.info('%d spectra identified after the open search', n_identified)   # :257
        out = SSMTable.concat([t1, t2])
        if cfg.chimeric_search:             # one more level on what the winners leave; off: nothing is launched
            out = self._chimeric_level(out, query_spectra, query_meta, library_meta, score_ssms, uid, n_identified)
        if cfg.localize_modifications:      # a post-step on the identifications; off: nothing is launched
            self.localize_modifications(out, query_spectra)
        return out

    def localize_modifications(self, table: 'SSMTable', query_spectra: Dict[int, PackedSpectra]) -> 'SSMTable':
        """Fill the ``mod_*`` columns of ``table`` (in place; also returned): for every SSM of the open
        cascade level whose precursor mass difference ``table.mass_diffs()`` passes the shift gate of the
        rescoring (``|delta| >= fragment_mz_tolerance``, in ppm ``>= fragment_mz_tolerance * 1e-6 *`` the
        query's precursor m/z) and whose library row has a ``peptide`` of 2 .. 128 residues, the site of
        that mass on the peptide as the processed query spectrum ``query_spectra[charge][qrow]`` shows it
        (localize.py, 32 768 SSMs per kernel launch). The tolerance is ``fragment_mz_tolerance`` in
        ``fragment_tolerance_unit``; ppm here is of the THEORETICAL fragment m/z, as for the decoys, not of
        the query peak as in the dot product. A peptide that does not parse (an unknown modification name,
        say) is skipped: one warning per call names their number and the first. Every other SSM keeps the
        defaults (NaN, -1). One GPU: ``ValueError`` on a sharded library."""
        from . import localize as lz
        from .decoy_generator import parse_peptide
        d = getattr(self, '_dist', None)
        if d is not None and d.world > 1:
            raise ValueError('localize_modifications does not run on a sharded index')
        cfg = self.config
        if len(table) == 0:
            return table
        delta = table.mass_diffs()
        gate = float(cfg.fragment_mz_tolerance)
        if cfg.fragment_tolerance_unit == 'ppm':    # rescore.hip, rs_frag_tol at the shift gate
            gate = gate * 1e-6 * table._column(table.query_meta, table.qrow, 'precursor_mz', np.float64)
        wanted = np.nonzero(table.open_level & (np.abs(delta) >= gate))[0]
        parsed: Dict[str, object] = {}
        n_bad, first_bad = 0, None
        for z in np.unique(table.charge[wanted]):
            lm = table.library_meta[int(z)]
            rows, peps = [], []
            for i in wanted[table.charge[wanted] == z]:
                rec = lm[int(table.lib_row[i])]
                text = rec.get('peptide') if hasattr(rec, 'get') else rec['peptide']
                if text not in parsed:
                    try:
                        parsed[text] = parse_peptide(text, spectrum=rec['identifier'])
                    except ValueError as e:
                        parsed[text] = None
                        first_bad = first_bad or str(e)
                pep = parsed[text]
                if pep is None:
                    n_bad += 1
                elif 2 <= len(pep.sequence) <= lz.MAX_RESIDUES:
                    rows.append(int(i))
                    peps.append(pep)
            qs = query_spectra[int(z)]
            for b0 in range(0, len(rows), lz.BATCH):
                sel = np.asarray(rows[b0:b0 + lz.BATCH], np.int64)
                q = qs.select(torch.as_tensor(table.qrow[sel]))
                out = lz.localize_batch(q, *lz.peptide_arrays(peps[b0:b0 + lz.BATCH], [int(z)] * len(sel)),
                                        delta[sel], cfg.fragment_mz_tolerance, cfg.fragment_tolerance_unit,
                                        self.device)
                out = {k: _to_np(out[k]) for k in lz.SSM_KEYS}
                table.mod_mass[sel] = delta[sel]
                table.mod_site_lo[sel], table.mod_site_hi[sel] = out['best_lo'], out['best_hi']
                table.mod_site_score[sel] = out['best_score']
                table.mod_site_margin[sel] = out['best_score'] - out['runner_score']
                table.mod_site_gain[sel] = out['best_score'] - out['none_score']
        if n_bad:
            logging.warning('modification localisation skipped %d SSMs whose library peptide does not parse; '
                            'the first: %s', n_bad, first_bad)
        return table

    def _chimeric_level(self, table: 'SSMTable', query_spectra, query_meta, library_meta, score_ssms, uid,
                        n_identified: int = 0) -> 'SSMTable':
        """``Config.chimeric_search``: ``table`` followed by the SSMs of one more level on the residues of its
        accepted identifications (``q < fdr``). Per charge, the queries of those SSMs are depleted by their
        winners (chimeric.py, 32 768 SSMs per kernel launch; the flag word is the search's own) and the valid
        residues are searched through ``_search_cascade`` -- window path, never the ANN index, no peak shifts
        (the precursor offset inside an isolation window is no modification), the fragment tolerance unit
        honoured -- against the rows of the same charge whose precursor m/z lies in the query's
        ``isolation_window`` when every query of the charge has one, else within ``chimeric_window / 2`` of
        its precursor m/z. A residue whose best match is the primary's peptide again (``peptide``, else
        ``sequence`` of the library metadata; without either: the library row) is dropped before the scorer,
        which is called with mode ``'std'``. The new rows carry ``chimeric_rank`` 1 and
        ``explained_intensity`` = 1 - the depletion's ``kept_energy``; ``open_level`` is False, so they are
        not localised. Their peak matches index the RESIDUE's peaks. One GPU."""
        from . import chimeric
        d = getattr(self, '_dist', None)
        if d is not None and d.world > 1:
            raise ValueError('chimeric_search does not run on a sharded index')
        cfg = self.config
        accepted = np.nonzero(table.q < cfg.fdr)[0]
        flags = score_flags(cfg.allow_peak_shifts, cfg.fragment_tolerance_unit)
        lvl = CascadeLevel('chimeric', {}, {}, {}, shifts=False)
        primary, explained = {}, {}
        for z in query_spectra:
            idx = accepted[table.charge[accepted] == z]
            if len(idx) == 0 or z not in self.partitions:
                continue
            qs = query_spectra[z]
            qrows, lib_rows = table.qrow[idx], table.lib_row[idx].astype(np.int64)
            pack, src, energy = chimeric.residues(qs.select(torch.as_tensor(qrows)), self.partitions[z].spectra,
                                                  lib_rows, cfg.fragment_mz_tolerance, flags, cfg.min_peaks,
                                                  cfg.min_mz_range, self.device)
            if pack.n == 0:
                continue
            lvl.spectra[z], lvl.qrow[z], primary[z] = pack, qrows[src], lib_rows[src]
            explained[z] = 1.0 - energy[src].astype(np.float64)
            meta = query_meta.get(z) if hasattr(query_meta, 'get') else None
            iso = isolation_windows(meta, qs.n)
            lvl.windows[z] = (iso[lvl.qrow[z]] if iso is not None else
                              chimeric_window_intervals(_to_np(qs.precursor_mz)[lvl.qrow[z]], cfg.chimeric_window))
        if not lvl.spectra:         # nothing accepted, or no residue is a valid spectrum: no level, no scorer call
            logging.info('%d spectra identified after the chimeric search', n_identified)
            return table

        def peptide(z, row):
            rec = library_meta[z][int(row)]
            get = rec.get if hasattr(rec, 'get') else (lambda k: None)
            for name in ('peptide', 'sequence'):
                v = get(name)
                if v is not None:
                    return v
            return ('row', int(row))

        def other_peptide(z, sel, best):
            return np.fromiter((r >= 0 and peptide(z, r) != peptide(z, p) for r, p in zip(best, primary[z][sel])),
                               bool, len(best))
        lvl.keep = other_peptide
        rows = {z: np.arange(p.n, dtype=np.int64) for z, p in lvl.spectra.items()}
        t3 = self._search_cascade(query_spectra, query_meta, library_meta, rows, 'std', score_ssms, uid, level=lvl)
        t3.chimeric_rank[:] = 1
        for z in lvl.spectra:
            m = t3.charge == z
            order = np.argsort(lvl.qrow[z], kind='stable')      # (one accepted SSM per query of a charge set)
            t3.explained_intensity[m] = explained[z][order][np.searchsorted(lvl.qrow[z][order], t3.qrow[m])]
        n_identified += int((t3.q < cfg.fdr).sum())
        logging.info('%d spectra identified after the chimeric search', n_identified)
        return SSMTable.concat([table, t3])

    def _open_level_windows(self, qs: PackedSpectra, query_meta, charge: int) -> Optional[np.ndarray]:
        """The open level's per-query intervals for one charge set ([qs.n, 2] float64), or None for the
        symmetric window of ``precursor_tolerance_mass_open``: the queries' isolation windows when every
        query of the set has one, else the range of ``Config.precursor_window_open`` around each query."""
        d = getattr(self, '_dist', None)
        sharded = d is not None and d.world > 1
        meta = query_meta.get(charge) if hasattr(query_meta, 'get') else None
        iso = isolation_windows(meta, qs.n)
        if iso is None and self.config.precursor_window_open is None:
            return None
        if sharded:     # like every other opt-in: an error, never another window than the one asked for
            raise ValueError(('isolation windows in the query metadata do' if iso is not None else
                              'precursor_window_open does') + ' not run on a sharded index')
        if iso is not None:
            return iso
        return open_window_intervals(_to_np(qs.precursor_mz), charge, self.config.precursor_window_open)

    def _search_cascade(self, query_spectra, query_meta, library_meta, rows_by_charge, mode,
                        score_ssms=None, uid=None, level: Optional['CascadeLevel'] = None) -> 'SSMTable':
        """One cascade level (:264-326): batches of ``batch_size`` same-charge queries through
        ``_search_batch``; per query identifier the FIRST match is kept (the reference compares
        ``search_engine_score`` values that are still NaN at this point, :312-316, so a later
        duplicate never replaces an earlier one). Host work is per batch, not per query.
        ``level``: None for the reference's two levels, or what a further level changes (``CascadeLevel``):
        the spectra it searches in place of ``query_spectra`` (``rows_by_charge`` then index those), their
        rows in ``query_spectra`` / ``query_meta`` for the table, their precursor intervals, the peak shifts
        and which matches never reach the scorer. ``mode`` stays what the batches and the scorer are given."""
        import time
        from . import spectrum_similarity
        bs = self.config.batch_size
        t_level = time.perf_counter()
        n_in = sum(len(r) for r in rows_by_charge.values())
        n_best = int(self.config.num_matches)
        distinct = bool(self.config.distinct_matches) and n_best > 1
        stats = bool(getattr(self.config, 'score_stats', False))
        table = SSMTable(query_meta, library_meta, n_best - 1)
        # Phase 1 issues every batch of the level; on one GPU the open-search batches go through
        # the two-stream pipeline (front of batch i+1 under the scan of batch i, no host wait
        # between batches). Phase 2, after one synchronisation, scores the winners and files them.
        d = getattr(self, '_dist', None)
        # (num_matches > 1, score_stats: the top-n entry points are synchronous, the batches are not pipelined)
        piped = (self.device.type == 'cuda' and (d is None or d.world == 1) and n_best == 1 and not stats and
                 not getattr(self, '_pipeline_on', False) and getattr(self, 'pipeline_cascade', True) and
                 any(self._uses_ann(z, mode) for z in rows_by_charge))
        if piped:
            self.set_pipeline(True)
        pending = []
        try:
            for charge, rows in rows_by_charge.items():
                rows = np.asarray(rows, np.int64)
                qs = query_spectra[charge] if level is None else level.spectra[charge]
                # open level: per-query intervals instead of the symmetric window (isolation windows of the
                # queries' metadata, else Config.precursor_window_open); None: the level's tolerance
                if level is not None:
                    level_win = level.windows[charge]
                else:
                    level_win = self._open_level_windows(qs, query_meta, charge) if mode == 'open' else None
                # (no keyword without a level: the signatures of older overrides keep working)
                more = {} if level is None else dict(shifts=level.shifts)
                for b0 in range(0, len(rows), bs):
                    sel = rows[b0:b0 + bs]
                    if len(sel) == 0:
                        continue
                    whole = len(sel) == qs.n and sel[0] == 0 and sel[-1] == qs.n - 1
                    q = (qs if whole else qs.select(torch.as_tensor(sel))).to(self.device)
                    win = None if level_win is None else level_win[sel]
                    if stats:           # the histogram call, at num_matches = 1 too
                        top = self.search_batch_topn(q, charge, mode, n_best, device_out=True,
                                                     distinct=distinct, windows=win, score_hist=True, **more)
                        res = None if top is None else top.rank0()
                        if res is not None:
                            res.topn = top
                    elif n_best > 1:    # rank 0 goes the single winner's way, the rest rides along
                        top = self.search_batch_topn(q, charge, mode, n_best, device_out=True,
                                                     distinct=distinct, windows=win, **more)
                        res = None if top is None else top.rank0()
                        if res is not None:
                            res.topn = top
                    else:
                        # (no keyword without windows: engines that override _search_batch with its older
                        # signature, as the oracle-backed ones of the tests do, keep working)
                        res = (self._search_batch(q, charge, mode, device_out=True) if win is None else
                               self._search_batch(q, charge, mode, device_out=True, windows=win, **more))
                    if res is not None:
                        pending.append((charge, sel, q, res))
        finally:
            if piped:
                self.set_pipeline(False)         # synchronises first
        def filed(charge, sel, res):
            """(charge, rows of query_spectra, winners) as the table files a batch: a further level names its
            queries by their rows in query_spectra and withholds the matches it drops (row -1: no SSM)."""
            best = _to_np(res.best_row)
            if level is None:
                return charge, sel, best
            qrows = level.qrow[charge][sel]
            if level.keep is not None:
                best = np.where(level.keep(charge, sel, best), best, -1).astype(best.dtype)
            return charge, qrows, best
        # default search-engine score: the cosine over the winner's peak matches -- every batch's
        # kernel is enqueued before the first result is copied back (a copy waits for its kernel)
        if getattr(score_ssms, 'uses_features', False):
            # a scorer that learns from the SSMs (fdr.PercolatorTDC): all 33 similarity columns of every batch;
            # column 0 has the bits of ssm_cosine, so the score does not change
            cfg = self.config
            feats = [spectrum_similarity.ssm_features(q, self.partitions[charge].spectra, res.best_row,
                                                      res.pm_pairs, res.pm_count, cfg.min_mz, cfg.max_mz,
                                                      cfg.bin_size)
                     for charge, sel, q, res in pending]
            for (charge, sel, q, res), F in zip(pending, feats):
                F = _to_np(F)
                table.add_batch(*filed(charge, sel, res), F[:, 0], res, F)
        else:
            cosines = [spectrum_similarity.ssm_cosine(q, self.partitions[charge].spectra, res.best_row,
                                                      res.pm_pairs, res.pm_count)
                       for charge, sel, q, res in pending]
            for (charge, sel, q, res), cos in zip(pending, cosines):
                table.add_batch(*filed(charge, sel, res), _to_np(cos), res)
        table.open_level[:] = mode == 'open'
        if uid is not None:
            table = table.first_per_uid(uid)
        acc = getattr(self, 'level_seconds', None)
        if acc is not None:       # bench.py: wall time, queries in, SSMs out of every cascade level
            torch.cuda.synchronize() if self.device.type == 'cuda' else None
            key = mode if level is None else level.name
            sec, a, b = acc.get(key, (0.0, 0, 0))
            acc[key] = (sec + time.perf_counter() - t_level, a + n_in, b + len(table))
        if score_ssms is None:    # no scorer: cosine (spectrum_similarity.py:81-106), accepted
            cascade = self.config.precursor_tolerance_mass_open is not None
            if (cascade or self.config.model is not None) and not getattr(self, '_warned_model', False):
                # the reference gates level 1 by utils.score_ssms (model or the `--model none`
                # FDR filter); without a scorer level 1 keeps EVERY query that had a
                # standard-window candidate, so the open level only sees the rest
                self._warned_model = True
                logging.warning('no score_ssms callable was given (model=%r): the FDR gate '
                                '(utils.score_ssms / mokapot) stays with the caller; every SSM is '
                                'accepted with its cosine as the score and q = 0%s',
                                self.config.model,
                                ', so the cascade hands only the queries without any '
                                'standard-window candidate to the open search' if cascade else '')
            table.q[:] = 0.0
            return table
        if getattr(score_ssms, 'columnar', False):
            keep = score_ssms(table, mode)
            return table if keep is None else table.take(np.asarray(keep))
        objs = table.materialize()
        for i, o in enumerate(objs):
            o._row = i
        kept = list(score_ssms(objs, mode))
        out = table.take(np.asarray([o._row for o in kept], np.int64))
        out.score = np.asarray([o.search_engine_score for o in kept], np.float64)
        out.q = np.asarray([o.q for o in kept], np.float64)
        return out


def _to_np(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def _cat_features(blocks) -> np.ndarray:
    """``SSMTable.features`` of several row blocks: [len, 33], or [len, 0] when none carries the columns (a
    block without them under one with them, an empty level say, is NaN)."""
    width = max(b.shape[1] for b in blocks)
    return np.concatenate([b if b.shape[1] == width else np.full((len(b), width), np.nan) for b in blocks])


def open_window_intervals(precursor_mz, charge: int, window_da) -> np.ndarray:
    """``Config.precursor_window_open`` as intervals of library precursor m/z, [n, 2] float64: the neutral
    mass difference (query - library) * charge lies in [lo_da, hi_da] iff the library's m/z lies in
    [q - hi_da / charge, q - lo_da / charge] (computed in float64; the bounds are inclusive)."""
    lo_da, hi_da = (float(v) for v in window_da)
    q = np.asarray(precursor_mz, np.float64)
    return np.stack([q - hi_da / charge, q - lo_da / charge], axis=1)


def chimeric_window_intervals(precursor_mz, width) -> np.ndarray:
    """``Config.chimeric_window`` as intervals of library precursor m/z, [n, 2] float64: [q - width / 2,
    q + width / 2] around every query's precursor m/z (computed in float64; the bounds are inclusive)."""
    q = np.asarray(precursor_mz, np.float64)
    half = float(width) / 2.0
    return np.stack([q - half, q + half], axis=1)


@dataclass
class CascadeLevel:
    """What a cascade level beyond the reference's two hands ``_search_cascade``: the spectra it searches, per
    charge, in place of the queries (residues, say); ``qrow[charge][i]``, the row of ``query_spectra`` /
    ``query_meta`` spectrum ``i`` stands for in the table; ``windows[charge]``, one closed interval of library
    precursor m/z per spectrum ([n, 2] float64: the candidates, as ``_search_batch(windows=)`` takes them);
    whether the dot product shifts peaks; ``keep(charge, rows, best_row) -> bool mask``, the winners that
    reach the table and the scorer (None: all); ``name``, its key in ``level_seconds``."""
    name: str
    spectra: Dict[int, PackedSpectra]
    qrow: Dict[int, np.ndarray]
    windows: Dict[int, np.ndarray]
    shifts: bool = False
    keep: Optional[object] = None


def isolation_windows(meta, n: int) -> Optional[np.ndarray]:
    """The queries' isolation windows, [n, 2] float64 (lo, hi) in m/z, from the optional ``isolation_window``
    entry of their metadata records -- None unless every one of the n queries has one. An entry that is no
    pair lo <= hi is a ValueError."""
    if meta is None or n == 0 or len(meta) < n:
        return None
    out = np.empty((n, 2), np.float64)
    for i in range(n):
        m = meta[i]
        w = m.get('isolation_window') if hasattr(m, 'get') else None
        if w is None:
            return None
        w = np.asarray(w, np.float64)
        if w.shape != (2,) or not w[0] <= w[1]:       # (a NaN bound fails too)
            raise ValueError(f'query {i}: isolation_window = {m.get("isolation_window")!r}; a pair (lo, hi) of m/z '
                             'with lo <= hi')
        out[i] = w
    return out


def _query_uids(query_meta, charges) -> Optional[Dict[int, np.ndarray]]:
    """Integer id per query identifier, shared across the charge sets -- or None when there is
    a single set (identifiers are unique inside a set, so nothing can collide)."""
    if len(charges) <= 1:
        return None
    table: Dict = {}
    out = {}
    for z in charges:
        out[z] = np.fromiter((table.setdefault(m['identifier'], len(table)) for m in query_meta[z]),
                             np.int64, len(query_meta[z]))
    return out


class SSMTable:
    """Spectrum-spectrum matches of a cascade level / the identifications of a search, columnar:
    ``charge``, ``qrow`` (row inside ``query_spectra[charge]``), ``lib_row`` (row inside the
    charge partition), ``score`` (search_engine_score), ``q``. Behaves as a sequence of the
    reference's SSM records (``spectrum.SpectrumSpectrumMatch``: the attributes writer.py:129-148
    reads), built on access from the query / library metadata and the peak matches the device
    emitted (kept per batch, fetched from the device when first needed).

    With ``num_matches = n > 1`` (``n_alt = n - 1``) every match also carries its runners-up:
    ``alt_lib_row[len, n_alt]`` (-1 padded) and ``alt_score[len, n_alt]`` (shifted-dot scores of
    ranks 1..), ``delta_score[len]`` (the rank-0 shifted-dot score minus rank 1's; the rank-0 score
    itself without a runner-up; NaN when ``n_alt = 0``) and ``alt_peak_matches(i, r)``.
    With ``distinct_matches`` the ranks are distinct identifications: ``alt_lib_row`` / ``alt_score``
    / ``alt_peak_matches`` name the best library spectrum of each of the next ``n_alt`` OTHER
    peptides (never another spectrum of the winner's or of an earlier runner-up's peptide), and
    ``delta_score`` is the gap to the best match of a different peptide.

    With ``score_stats`` every match carries ``n_scored[len]``, the candidates its query scored, and
    ``expect[len]``, how many of them were expected to score at least as high as the match by chance
    (``score_stats.expect_value`` over the batch's score histograms; NaN where no tail could be fitted:
    fewer than 10 losers, fewer than 3 fit points, a slope that is not negative). Without the option
    the columns hold 0 and NaN.

    ``open_level[len]`` says which matches come from the open cascade level. With ``localize_modifications``
    (``SpectralLibrary.localize_modifications``) those with a real precursor mass difference carry where the
    query's peaks put it on the library peptide: ``mod_mass`` (the mass, Da), ``mod_site_lo`` /
    ``mod_site_hi`` (first and last of the equally best sites, 0-based residue indices),
    ``mod_site_score`` (the summed intensity of the best site's plain and shifted b / y fragments),
    ``mod_site_margin`` (best minus the best different score; 0 when every site ties) and ``mod_site_gain``
    (best minus the score without the mass). Everywhere else: NaN and -1.

    With ``chimeric_search`` the table ends with the matches of the residue level: ``chimeric_rank`` 1 (0 for
    everything else) and ``explained_intensity``, the share of the query's squared intensity its PRIMARY match
    explains (NaN on rank-0 rows). Such a row names the same query as a rank-0 row: the table may hold two SSMs
    for one identifier, and the peak matches of the second index the residue spectrum's peaks.

    ``features[len, 33]`` (float64) holds the similarity columns of ``spectrum_similarity.FEATURE_NAMES`` when
    the level ran for a scorer that learns from them (``fdr.PercolatorTDC``); ``[len, 0]`` otherwise."""

    # columns that are filled after the batches are filed: (name, dtype, default)
    _LATE = (('open_level', bool, False), ('mod_mass', np.float64, np.nan), ('mod_site_lo', np.int32, -1),
             ('mod_site_hi', np.int32, -1), ('mod_site_score', np.float64, np.nan),
             ('mod_site_margin', np.float64, np.nan), ('mod_site_gain', np.float64, np.nan),
             ('chimeric_rank', np.int32, 0), ('explained_intensity', np.float64, np.nan))

    def __init__(self, query_meta, library_meta, n_alt: int = 0):
        self.query_meta, self.library_meta = query_meta, library_meta
        self.n_alt = int(n_alt)
        self.alt_lib_row = np.zeros((0, self.n_alt), np.int32)
        self.alt_score = np.zeros((0, self.n_alt), np.float64)
        self.delta_score = np.zeros(0, np.float64)
        self.n_scored = np.zeros(0, np.int32)
        self.expect = np.zeros(0, np.float64)
        self.features = np.zeros((0, 0), np.float64)
        self._alt_batches: list = []             # per batch: its TopnBatchResult (None: single winner)
        self.charge = np.zeros(0, np.int32)
        self.qrow = np.zeros(0, np.int64)
        self.lib_row = np.zeros(0, np.int32)
        self.score = np.zeros(0, np.float64)
        self.q = np.zeros(0, np.float64)
        self.batch = np.zeros(0, np.int32)       # index into _batches
        self.pos = np.zeros(0, np.int32)         # row inside that batch
        self._batches: list = []
        self._pending: list = []
        for name, dt, _ in self._LATE:
            setattr(self, name, np.zeros(0, dt))

    def add_batch(self, charge, qrows, best_row, score, res, features=None) -> None:
        hit = np.nonzero(best_row >= 0)[0]       # queries without a candidate: no SSM (:359)
        feats = np.zeros((len(hit), 0)) if features is None else np.asarray(features, np.float64)[hit]
        self.features = _cat_features([self.features, feats])
        b = len(self._batches)
        self._batches.append(res)
        top = getattr(res, 'topn', None)
        self._alt_batches.append(top)
        alt_row = np.full((len(hit), self.n_alt), -1, np.int32)
        alt_score = np.zeros((len(hit), self.n_alt), np.float64)
        delta = np.full(len(hit), np.nan)
        if top is not None and self.n_alt > 0:
            rows, scores = _to_np(top.best_row)[hit], _to_np(top.best_score)[hit]
            alt_row, alt_score = rows[:, 1:].astype(np.int32), scores[:, 1:].astype(np.float64)
            delta = scores[:, 0] - scores[:, 1]      # (an empty rank's score is 0.0)
        self.alt_lib_row = np.concatenate([self.alt_lib_row, alt_row])
        self.alt_score = np.concatenate([self.alt_score, alt_score])
        self.delta_score = np.concatenate([self.delta_score, delta])
        n_scored, expect = np.zeros(len(hit), np.int32), np.full(len(hit), np.nan)
        if top is not None and getattr(top, 'score_hist', None) is not None:
            from . import score_stats
            best = _to_np(top.best_score)[hit, 0]
            n_scored = _to_np(top.n_candidates)[hit].astype(np.int32)
            expect = score_stats.expect_value(score_stats.loser_hist(_to_np(top.score_hist)[hit], best), best)
        self.n_scored = np.concatenate([self.n_scored, n_scored])
        self.expect = np.concatenate([self.expect, expect])
        self._pending.append((np.full(len(hit), charge, np.int32), np.asarray(qrows, np.int64)[hit],
                              best_row[hit].astype(np.int32), np.asarray(score, np.float64)[hit],
                              np.full(len(hit), b, np.int32), hit.astype(np.int32)))
        self._flush()

    def _flush(self):
        if not self._pending:
            return
        cols = list(zip(*self._pending))
        self._pending = []
        cat = lambda old, new: np.concatenate([old] + list(new))
        self.charge, self.qrow = cat(self.charge, cols[0]), cat(self.qrow, cols[1])
        self.lib_row, self.score = cat(self.lib_row, cols[2]), cat(self.score, cols[3])
        self.batch, self.pos = cat(self.batch, cols[4]), cat(self.pos, cols[5])
        self.q = np.concatenate([self.q, np.full(len(self.charge) - len(self.q), np.nan)])
        for name, dt, default in self._LATE:
            old = getattr(self, name)
            setattr(self, name, np.concatenate([old, np.full(len(self.charge) - len(old), default, dt)]))

    def __len__(self):
        return len(self.charge)

    def take(self, sel) -> 'SSMTable':
        """Rows ``sel`` (boolean mask or indices, order kept); shares the per-batch storage."""
        sel = np.asarray(sel)
        idx = np.nonzero(sel)[0] if sel.dtype == bool else sel.astype(np.int64)
        out = SSMTable(self.query_meta, self.library_meta, self.n_alt)
        out._batches, out._alt_batches = self._batches, self._alt_batches
        for name in ('charge', 'qrow', 'lib_row', 'score', 'q', 'batch', 'pos', 'alt_lib_row', 'alt_score',
                     'delta_score', 'n_scored', 'expect', 'features') + tuple(c[0] for c in self._LATE):
            setattr(out, name, getattr(self, name)[idx])
        return out

    @staticmethod
    def concat(tables) -> 'SSMTable':
        out = SSMTable(tables[0].query_meta, tables[0].library_meta, max(t.n_alt for t in tables))
        shift = 0
        for t in tables:
            out._batches = out._batches + t._batches
            out._alt_batches = out._alt_batches + t._alt_batches
            pad = ((0, 0), (0, out.n_alt - t.n_alt))
            out.alt_lib_row = np.concatenate([out.alt_lib_row, np.pad(t.alt_lib_row, pad, constant_values=-1)])
            out.alt_score = np.concatenate([out.alt_score, np.pad(t.alt_score, pad)])
            for name in ('charge', 'qrow', 'lib_row', 'score', 'q', 'pos', 'delta_score', 'n_scored',
                         'expect') + tuple(c[0] for c in SSMTable._LATE):
                setattr(out, name, np.concatenate([getattr(out, name), getattr(t, name)]))
            out.batch = np.concatenate([out.batch, t.batch + shift])
            shift += len(t._batches)
        out.features = _cat_features([t.features for t in tables])
        return out

    def uids(self, uid) -> np.ndarray:
        out = np.zeros(len(self), np.int64)
        for z in np.unique(self.charge):
            m = self.charge == z
            out[m] = uid[int(z)][self.qrow[m]]
        return out

    def first_per_uid(self, uid) -> 'SSMTable':
        u = self.uids(uid)
        _, first = np.unique(u, return_index=True)
        return self if len(first) == len(u) else self.take(np.sort(first))

    def identifiers(self) -> list:
        return [self.query_meta[int(z)][int(r)]['identifier'] for z, r in zip(self.charge, self.qrow)]

    def library_identifiers(self, partitions) -> np.ndarray:
        """Library identifiers of the matches (``partitions``: ``SpectralLibrary.partitions``)."""
        out = np.empty(len(self), dtype=object)
        for z in np.unique(self.charge):
            m = self.charge == z
            out[m] = partitions[int(z)].ids[self.lib_row[m]]
        return out

    def _column(self, meta, rows, name, dtype, default=None) -> np.ndarray:
        """One metadata attribute of the matches as an array. A metadata container may offer
        ``column(name, rows)`` (arrays behind it) -- otherwise it is read record by record."""
        out = np.zeros(len(self), dtype)
        for z in np.unique(self.charge):
            m = self.charge == z
            cont, r = meta[int(z)], rows[m]
            if hasattr(cont, 'column'):
                out[m] = cont.column(name, r)
            elif default is None:
                out[m] = [cont[int(i)][name] for i in r]
            else:
                out[m] = [cont[int(i)].get(name, default) for i in r]
        return out

    def is_decoy(self) -> np.ndarray:
        return self._column(self.library_meta, self.lib_row, 'is_decoy', bool, False)

    def mass_diffs(self) -> np.ndarray:
        """(experimental - library precursor m/z) * query charge, the quantity the reference
        groups open-search SSMs by (utils.py:227-232)."""
        exp = self._column(self.query_meta, self.qrow, 'precursor_mz', np.float64)
        z = self._column(self.query_meta, self.qrow, 'precursor_charge', np.float64)
        calc = self._column(self.library_meta, self.lib_row, 'precursor_mz', np.float64)
        return (exp - calc) * z

    def _peak_matches(self, i) -> np.ndarray:
        b = self._batches[int(self.batch[i])]
        if not isinstance(b, tuple):             # first access: one device -> host copy per batch
            b = (_to_np(b.pm_count), _to_np(b.pm_pairs))
            self._batches[int(self.batch[i])] = b
        p = int(self.pos[i])
        return b[1][p, :b[0][p]].astype(np.int64)

    def alt_peak_matches(self, i, r) -> np.ndarray:
        """Peak matches ``[n, 2]`` of match ``i``'s rank ``r`` (1 .. n_alt) runner-up; empty when
        the query had no such rank."""
        if not 1 <= r <= self.n_alt:
            raise IndexError(f'rank {r}: this table holds ranks 1 .. {self.n_alt}')
        b = self._alt_batches[int(self.batch[i])]
        if b is None:
            return np.zeros((0, 2), np.int64)
        if not isinstance(b, tuple):             # first access: one device -> host copy per batch
            b = (_to_np(b.pm_count), _to_np(b.pm_pairs))
            self._alt_batches[int(self.batch[i])] = b
        p = int(self.pos[i])
        return b[1][p, r, :b[0][p, r]].astype(np.int64)

    def _alternatives(self, i) -> tuple:
        lm = self.library_meta[int(self.charge[i])]
        return tuple((lm[int(row)]['identifier'], float(self.alt_score[i, r]), self.alt_peak_matches(i, r + 1))
                     for r, row in enumerate(self.alt_lib_row[i]) if row >= 0)

    def __getitem__(self, i):
        from .spectrum import SpectrumSpectrumMatch
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        z = int(self.charge[i])
        qm, lm = self.query_meta[z][int(self.qrow[i])], self.library_meta[z][int(self.lib_row[i])]
        return SpectrumSpectrumMatch(
            lm['peptide'], qm['identifier'], qm['index'], lm['identifier'],
            qm.get('retention_time'), qm['precursor_charge'], qm['precursor_mz'],
            lm['precursor_mz'], lm.get('is_decoy', False), float(self.score[i]), float(self.q[i]),
            self._peak_matches(i), float(self.delta_score[i]), self._alternatives(i),
            int(self.n_scored[i]), float(self.expect[i]), float(self.mod_mass[i]), int(self.mod_site_lo[i]),
            int(self.mod_site_hi[i]), float(self.mod_site_score[i]), float(self.mod_site_margin[i]),
            float(self.mod_site_gain[i]), int(self.chimeric_rank[i]), float(self.explained_intensity[i]))

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def materialize(self) -> list:
        return list(self)
