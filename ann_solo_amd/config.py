"""The options that reach the hot path.

``Config`` carries the reference's flags under the reference's names
(/root/reference/src/ann_solo/config.py:62-216) plus the ADDITIVE flags of this implementation
(``index``, ``pq_m``, ``pq_bits``, ``refine_k``, ``kmeans_niter``, ``ann_seed``, ``num_gpus``,
``flat_storage``, ``ann_window``, ``num_matches``, ``distinct_matches``, ``pq_by_residual``,
``precursor_window_open``, ``fragment_tolerance_unit``, ``score_stats``, ``device_decoys``,
``decoy_tolerance_unit``, ``localize_modifications``, ``device_fdr``, ``device_forest``,
``forest_trees``, ``device_qvalues``, ``device_groups``, ``chimeric_search``, ``chimeric_window``,
``device_mgf``, ``device_mzml``, ``device_mzxml``, ``device_library``). Defaults are the reference's: ``precursor_tolerance_mass_open`` /
``_mode_open`` are ``None`` (cascade off, config.py:151-156) and ``allow_peak_shifts`` is False
(a ``store_true`` flag, config.py:157), as a parsed reference configuration without those flags
has them. The one deviation: ``precursor_tolerance_mass`` / ``precursor_tolerance_mode`` /
``fragment_mz_tolerance`` are REQUIRED by the reference's parser (config.py:137-150) and default
here to 20 ppm / 0.02 Da, the values of the reference's notebooks. ``Config.open_search(**kw)``
is the hand-built configuration the tests and ``bench.py`` use: the notebooks' open search
(+-300 Da second cascade level, notebooks/iprg2012_ann_hyperparameters.ipynb:100-101) with peak
shifts on. ``tests/ref_config.py`` holds the reference's own defaults; ``Config.from_reference``
takes every value from the parsed reference object.

Capacity limits of the device kernels are checked at construction (``ValueError``), not deep
inside a search: ``max_peaks_used`` / ``max_peaks_used_library`` <= 256 (the reference has no
limit; its default is 50), ``num_probe`` <= 2048, ``num_candidates`` <= 16 384 (beyond 2 048 the
search runs ceil(k / 2048) bounded passes of the generic kernels: exact, slower).
``Config.from_reference(obj)`` snapshots any configuration object -- in particular the
reference's own ``ann_solo.config.config`` singleton, whose ``__getattr__`` answers unknown
options with ``KeyError`` (config.py:285-291), not ``AttributeError`` -- so the engine can be
constructed exactly as ``ann_solo.py:78-79`` does. ``add_arguments(parser)`` is the additive
patch for the reference's ``Config.__init__``."""
from dataclasses import dataclass, fields
from typing import Optional, Tuple

_MISSING = object()


@dataclass
class Config:
    # --- the reference's flags (config.py:62-216), same names; defaults: see the module docstring
    resolution: Optional[int] = None
    min_mz: int = 11
    max_mz: int = 2010
    remove_precursor: bool = False
    remove_precursor_tolerance: float = 0
    min_intensity: float = 0.01
    min_peaks: int = 10
    min_mz_range: float = 250
    max_peaks_used: int = 50
    max_peaks_used_library: int = 50
    scaling: Optional[str] = 'rank'
    fdr: float = 0.01
    fdr_min_group_size: int = 100
    spectral_library_filename: str = ''
    query_filename: str = ''
    out_filename: str = ''
    bin_size: float = 0.04
    hash_len: int = 800
    num_candidates: int = 1024
    batch_size: int = 16384
    num_list: int = 256
    num_probe: int = 128
    mode: str = 'ann'                       # 'ann' | 'bf'
    precursor_tolerance_mass: float = 20.0
    precursor_tolerance_mode: str = 'ppm'   # 'Da' | 'ppm'
    precursor_tolerance_mass_open: Optional[float] = None
    precursor_tolerance_mode_open: Optional[str] = None
    fragment_mz_tolerance: float = 0.02
    allow_peak_shifts: bool = False
    no_gpu: bool = False
    # SSM scoring (config.py:158-164): carried for the caller's scorer, ``score_ssms=``; without one every
    # SSM is accepted with its cosine as the score and q = 0 -- unless ``device_fdr`` (below) is set, which
    # makes the engine build its own scorer from this value.
    model: Optional[str] = None
    # --- additive flags of this implementation
    index: str = 'ivfflat'                  # 'ivfflat' (the reference's index type) | 'ivfpq' | 'winflat' (exact
                                            # inner products over every library vector of the query's precursor
                                            # window: no coarse quantiser; num_list / num_probe are ignored)
    pq_m: int = 32
    pq_bits: int = 8
    refine_k: Optional[int] = None          # IVF-PQ: exact re-rank of the refine_k best ADC candidates
    kmeans_niter: int = 25                  # FAISS' ClusteringParameters.niter default
    seed: int = 1234                        # flag --ann_seed; FAISS' ClusteringParameters.seed default
    num_gpus: int = 0                       # > 1: list-shard the ANN indexes over that many ranks
    flat_storage: str = 'fp32'              # IVF-Flat component storage: 'fp32' (as given: the reference's
                                            # CPU index) | 'fx22' (opt-in: 22-bit fixed point for
                                            # components in [0, 1), 4-byte postings, |dx| <= 1.2e-7)
    ann_window: str = 'post'                # open search: 'post' (the reference's order: k best of the probed
                                            # lists, then the precursor window) | 'pre' (opt-in, IVF-PQ: the k
                                            # best in-window vectors of the probed lists)
    num_matches: int = 1                    # library matches reported per query: 1 (the reference: the best
                                            # match) .. 16; > 1 adds the runners-up and the score gap to the
                                            # SSMs (top-n rescoring), identifications and FDR stay rank 0's
    distinct_matches: bool = False          # num_matches > 1: the runners-up are the best matches of OTHER
                                            # peptides (one rank per peptide; the score gap is the gap to the
                                            # next different identification), not other spectra of the winner's

    pq_by_residual: bool = True             # IVF-PQ, FAISS' IndexIVFPQ.by_residual: True codes the residuals
                                            # x - centroid[list]; False (opt-in) the hashed vectors themselves
    # open cascade level: the signed range (lo_da, hi_da) of the neutral mass difference (query - library) *
    # charge a candidate may have, e.g. (-150, 500), instead of the symmetric +-precursor_tolerance_mass_open
    # (flags --precursor_window_open_low / _high). None: the reference's symmetric window
    precursor_window_open: Optional[Tuple[float, float]] = None
    # unit of fragment_mz_tolerance in the (shifted) dot product: 'Da' (the reference: one window width for
    # every peak) | 'ppm' (opt-in: of the QUERY peak's m/z, tol_i = tolerance * 1e-6 * q_mz[i]).
    # Deliberately NOT the reference's ``fragment_tol_mode``: that flag defaults to 'ppm' but reaches only the
    # decoy annotation -- the reference's dot product reads the tolerance as Da whatever it says -- so
    # ``from_reference`` would pick its default up and change the results of every existing configuration.
    fragment_tolerance_unit: str = 'Da'
    # every SSM also says how many candidates its query scored (n_scored) and how many of them were expected
    # to score as high as the winner by chance (expect: a log-linear fit to the tail of the losers' score
    # histogram, which the device counts; score_stats.py). Identifications, scores and files do not change
    score_stats: bool = False
    # make a shuffle-and-reposition decoy of every library spectrum on the device while the library is read
    # (decoy_generator.py; DESIGN.md 3 "Decoys"): the library then holds decoy and target rows in pairs. The
    # annotation tolerance is fragment_mz_tolerance in decoy_tolerance_unit, the shuffle's key is ``seed``.
    # Deliberately NOT the reference's ``add_decoys``: its own reader honours that flag from its global
    # configuration, and picking it up through ``from_reference`` would add decoys twice.
    device_decoys: bool = False
    # 'ppm' (of the theoretical fragment m/z) | 'Da'. The default is the default of the reference's
    # ``fragment_tol_mode``, which reaches its decoy annotation only; this is the one place it is read
    decoy_tolerance_unit: str = 'ppm'
    # after the search, say for every open-level identification with a real precursor mass difference which
    # residue of the library peptide the query's peaks put that mass on (localize.py; DESIGN.md 3
    # "Localisation"): the SSMs' mod_* columns. The tolerance is fragment_mz_tolerance in
    # fragment_tolerance_unit, ppm being of the THEORETICAL fragment m/z here. A post-step: identifications,
    # scores, FDR, files and every hash are what they are without it
    localize_modifications: bool = False
    # the engine's own FDR step (fdr.py; DESIGN.md 3 "Rescoring model"): without an injected ``score_ssms`` the
    # cascade levels are gated by ``model`` -- None / 'none': target-decoy q-values on the cosine; 'svm': a
    # Percolator-like linear SVM over the reference's feature table, trained on the device -- at ``fdr``, open
    # level grouped with ``fdr_min_group_size``. 'rf' alone is not provided (ValueError; see device_forest). An injected callable always
    # wins; off: every SSM is accepted with q = 0, as ever
    device_fdr: bool = False
    # with device_fdr and model = 'rf': the engine's histogram forest (fdr.ForestTDC, csrc/forest.hip; DESIGN.md 3
    # "Rescoring model: forest") of ``forest_trees`` trees per forest. A switch of its own because the forest is a
    # restatement -- binned splits, not scikit-learn's exact ones -- and must not silently stand for 'rf'
    device_forest: bool = False
    forest_trees: int = 100         # scikit-learn's n_estimators default; 1 .. MAX_FOREST_TREES
    # with device_fdr: the scorers' target-decoy q-values -- the relabelling of every round, the held-out part,
    # the grouped step -- by ``asl_tdc_qvalues`` on the device (csrc/tdc.hip; DESIGN.md 3 "Target-decoy q-values")
    # in place of numpy on the host; the same bytes either way. Off: nothing new is launched
    device_qvalues: bool = False
    # with device_fdr: the open level's mass-difference group labels by ``asl_ssm_groups`` on the device
    # (csrc/groups.hip; DESIGN.md 3 "Mass-difference groups") in place of ``fdr.ssm_groups`` on the host; the same
    # bytes either way, and the scorer keeps the modification profile (``group_profile``). Off: nothing new is launched
    device_groups: bool = False
    # chimeric spectra (chimeric.py; DESIGN.md 3 "Chimeric search"): after the last cascade level every accepted
    # identification's explained peaks are removed from its query and the residue is searched once more, without
    # peak shifts, against the library rows of the same charge inside the query's isolation window -- the
    # ``isolation_window`` of the query metadata, else ``chimeric_window`` (full width, m/z) around its precursor.
    # Matches of another peptide are appended with ``chimeric_rank`` 1. Off: nothing is launched and every
    # result, hash and output byte is what it is without the switch
    chimeric_search: bool = False
    chimeric_window: float = 2.0
    # ``SpectralLibrary.search(filename)`` reads a query file whose name ends in ``.mgf`` (any letter case) with
    # the engine's own reader (mgf.py, csrc/mgf.hip; DESIGN.md 3 "Query files"): the text is parsed by kernels and
    # the raw peaks go to the preprocessing where they lie, in place of ``query_reader`` and ``pack_queries``; the
    # same packed queries either way. Other extensions keep the injected or the reference's reader. Off: nothing
    # new is launched
    device_mgf: bool = False
    # The same for a query file whose name ends in ``.mzml`` (any letter case): the tags are parsed and the base64 /
    # zlib arrays decoded by kernels (mzml.py, csrc/mzml.hip, csrc/inflate.hpp; DESIGN.md 3 "Query files"), in place
    # of ``query_reader`` (the reference's pyteomics reader) and ``pack_queries``. Off: nothing new is launched
    device_mzml: bool = False
    # The same for a query file whose name ends in ``.mzxml`` (any letter case): nested scans, the precursor's element
    # text, ISO-8601 retention times and the one interleaved big-endian base64 / zlib stream of each MS2 scan are read
    # by kernels (mzxml.py, csrc/mzxml.hip; DESIGN.md 3 "Query files"). Off: nothing new is launched
    device_mzxml: bool = False
    # ``SpectralLibrary(filename)`` reads a library whose name ends in ``.sptxt`` (any letter case) with the engine's
    # own reader (sptxt.py, csrc/sptxt.hip; DESIGN.md 3 "Library files") in place of ``reader_factory``: the text is
    # parsed by kernels, the raw peaks go to the preprocessing where they lie, and the packed store is what
    # ``build_library_store`` makes of the same file. Other extensions keep the injected or the reference's reader.
    # Off: nothing new is launched and every result, hash and cached file name is what it is without the switch
    device_library: bool = False

    MAX_PEAKS = 256     # peaks per spectrum the preprocessing / rescoring kernels hold (csrc/process.hip)
    MAX_TOPK = 2048      # largest nprobe / single-pass k of the LDS top-k (csrc/ivf_kernels.hpp: TK_MAX_K)
    MAX_CANDIDATES = 16384   # largest num_candidates: beyond MAX_TOPK in bounded passes (TK_MAX_K_PASSES)
    MAX_MATCHES = 16     # largest num_matches (include/annsolo_mi.h: ASL_MAX_BEST)
    MAX_FOREST_TREES = 1024  # largest forest_trees (ASL_FOREST_MAX_TREES)

    def __post_init__(self):
        for name in ('max_peaks_used', 'max_peaks_used_library'):
            v = getattr(self, name)
            if v is not None and int(v) > self.MAX_PEAKS:
                raise ValueError(f'{name} = {v}: the device kernels hold at most {self.MAX_PEAKS} '
                                 'peaks per spectrum (the reference has no limit; its default is 50)')
        for name, lim in (('num_candidates', self.MAX_CANDIDATES), ('num_probe', self.MAX_TOPK)):
            v = getattr(self, name)
            if v is not None and int(v) > lim:
                raise ValueError(f'{name} = {v}: the device top-k holds at most {lim} entries')
        if self.flat_storage not in ('fx22', 'fp32'):
            raise ValueError(f"flat_storage = {self.flat_storage!r}: 'fx22' or 'fp32'")
        if self.ann_window not in ('post', 'pre'):
            raise ValueError(f"ann_window = {self.ann_window!r}: 'post' or 'pre'")
        if self.ann_window == 'pre':
            if self.index != 'ivfpq' or int(self.pq_m) != 32 or int(self.pq_bits) != 8:
                raise ValueError("ann_window = 'pre' needs index = 'ivfpq' with pq_m = 32, pq_bits = 8 "
                                 '(the window scan of the tiled IVF-PQ layout)')
            if self.num_gpus and int(self.num_gpus) > 1:
                raise ValueError("ann_window = 'pre' does not run on a sharded index (num_gpus > 1)")
            if self.refine_k:
                raise ValueError("ann_window = 'pre' does not combine with refine_k")
        self.pq_by_residual = bool(self.pq_by_residual)      # (the flag parses to 0 / 1)
        if self.index == 'winflat':
            if self.num_gpus and int(self.num_gpus) > 1:
                raise ValueError("index = 'winflat' does not run on a sharded index (num_gpus > 1)")
            if self.refine_k:
                raise ValueError("index = 'winflat' scores exactly already: it does not combine with refine_k")
            if self.num_candidates is not None and int(self.num_candidates) > 1280:
                raise ValueError(f"index = 'winflat' holds num_candidates <= 1280 (num_candidates = "
                                 f'{self.num_candidates})')
        if not self.pq_by_residual and self.index != 'ivfpq':
            raise ValueError("pq_by_residual = False needs index = 'ivfpq' (it is the product quantiser's mode)")
        if not 1 <= int(self.num_matches) <= self.MAX_MATCHES:
            raise ValueError(f'num_matches = {self.num_matches}: 1 .. {self.MAX_MATCHES}')
        if int(self.num_matches) > 1 and self.num_gpus and int(self.num_gpus) > 1:
            raise ValueError('num_matches > 1 does not run on a sharded index (num_gpus > 1)')
        if self.distinct_matches and self.num_gpus and int(self.num_gpus) > 1:
            raise ValueError('distinct_matches does not run on a sharded index (num_gpus > 1)')
        if self.fragment_tolerance_unit not in ('Da', 'ppm'):
            raise ValueError(f"fragment_tolerance_unit = {self.fragment_tolerance_unit!r}: 'Da' or 'ppm'")
        if self.fragment_tolerance_unit == 'ppm' and self.num_gpus and int(self.num_gpus) > 1:
            raise ValueError("fragment_tolerance_unit = 'ppm' does not run on a sharded index (num_gpus > 1)")
        self.score_stats = bool(self.score_stats)
        if self.score_stats and self.num_gpus and int(self.num_gpus) > 1:
            raise ValueError('score_stats does not run on a sharded index (num_gpus > 1)')
        self.device_decoys = bool(self.device_decoys)
        if self.decoy_tolerance_unit not in ('Da', 'ppm'):
            raise ValueError(f"decoy_tolerance_unit = {self.decoy_tolerance_unit!r}: 'Da' or 'ppm'")
        self.localize_modifications = bool(self.localize_modifications)
        if self.localize_modifications and self.num_gpus and int(self.num_gpus) > 1:
            raise ValueError('localize_modifications does not run on a sharded index (num_gpus > 1)')
        self.device_fdr = bool(self.device_fdr)
        self.device_forest = bool(self.device_forest)
        self.forest_trees = int(self.forest_trees)
        if not 1 <= self.forest_trees <= self.MAX_FOREST_TREES:
            raise ValueError(f'forest_trees = {self.forest_trees}: 1 .. {self.MAX_FOREST_TREES}')
        if self.device_forest:
            if not self.device_fdr or self.model != 'rf':
                raise ValueError("device_forest is the forest of the engine's own FDR step: it needs device_fdr "
                                 f"and model = 'rf' (device_fdr = {self.device_fdr}, model = {self.model!r})")
            if self.num_gpus and int(self.num_gpus) > 1:
                raise ValueError('device_forest does not run on a sharded index (num_gpus > 1)')
        if self.device_fdr:
            if self.model not in (None, 'none', 'svm') and not (self.model == 'rf' and self.device_forest):
                raise ValueError(f"device_fdr: model = {self.model!r} is not provided; None / 'none' (q-values on "
                                 "the cosine) or 'svm' (the Percolator-like linear SVM)")
            if self.num_gpus and int(self.num_gpus) > 1:
                # (a level's SSMs are gathered on rank 0 only after its gate)
                raise ValueError('device_fdr does not run on a sharded index (num_gpus > 1)')
        self.device_qvalues = bool(self.device_qvalues)
        if self.device_qvalues:
            if not self.device_fdr:
                raise ValueError("device_qvalues is the q-value step of the engine's own FDR step: it needs "
                                 f'device_fdr (device_fdr = {self.device_fdr})')
            if self.num_gpus and int(self.num_gpus) > 1:
                raise ValueError('device_qvalues does not run on a sharded index (num_gpus > 1)')
        self.device_groups = bool(self.device_groups)
        if self.device_groups:
            if not self.device_fdr:
                raise ValueError("device_groups is the grouping step of the engine's own FDR step: it needs "
                                 f'device_fdr (device_fdr = {self.device_fdr})')
            if self.num_gpus and int(self.num_gpus) > 1:
                raise ValueError('device_groups does not run on a sharded index (num_gpus > 1)')
        self.chimeric_search = bool(self.chimeric_search)
        self.chimeric_window = float(self.chimeric_window)
        if not self.chimeric_window >= 0.0:     # (NaN fails too)
            raise ValueError(f'chimeric_window = {self.chimeric_window}: a width in m/z, >= 0')
        if self.chimeric_search and self.num_gpus and int(self.num_gpus) > 1:
            raise ValueError('chimeric_search does not run on a sharded index (num_gpus > 1)')
        self.device_mgf = bool(self.device_mgf)
        self.device_mzml = bool(self.device_mzml)
        self.device_mzxml = bool(self.device_mzxml)
        self.device_library = bool(self.device_library)
        if self.precursor_window_open is not None:
            try:
                lo, hi = (float(v) for v in self.precursor_window_open)
            except (TypeError, ValueError):
                raise ValueError(f'precursor_window_open = {self.precursor_window_open!r}: a pair (lo_da, hi_da)')
            if not lo <= hi:        # (a NaN bound fails too)
                raise ValueError(f'precursor_window_open = ({lo}, {hi}): needs lo_da <= hi_da')
            if self.precursor_tolerance_mass_open is None:
                raise ValueError('precursor_window_open shapes the open cascade level: it needs '
                                 'precursor_tolerance_mass_open (the switch of that level)')
            if self.num_gpus and int(self.num_gpus) > 1:
                raise ValueError('precursor_window_open does not run on a sharded index (num_gpus > 1)')
            self.precursor_window_open = (lo, hi)

    def __getitem__(self, k):
        return getattr(self, k)

    @property
    def ann_seed(self) -> int:              # the flag's name on the command line
        return self.seed

    @classmethod
    def open_search(cls, **kw) -> 'Config':
        """A hand-built configuration with the open-modification search switched on the way the
        reference's notebooks run it: second cascade level +-300 Da, shifted dot product."""
        base = dict(precursor_tolerance_mass_open=300.0, precursor_tolerance_mode_open='Da',
                    allow_peak_shifts=True)
        base.update(kw)
        return cls(**base)

    @classmethod
    def from_reference(cls, obj, **overrides) -> 'Config':
        """Snapshot of ``obj`` (a ``Config``, the reference's ``config`` singleton, an
        ``argparse.Namespace``, a mapping ...): every field it answers is taken, every field it
        does not know (``KeyError`` / ``AttributeError`` / ``RuntimeError`` of an unparsed
        reference config is NOT swallowed) keeps the default above."""
        if isinstance(obj, cls) and not overrides:
            return obj
        kw = {}
        for f in fields(cls):
            v = _lookup(obj, 'ann_seed' if f.name == 'seed' else f.name)
            if v is _MISSING and f.name == 'seed':
                v = _lookup(obj, 'seed')
            if v is not _MISSING:
                kw[f.name] = v
        if 'precursor_window_open' not in kw:      # the two flags of add_arguments: both or neither
            lo, hi = (_lookup(obj, 'precursor_window_open_' + side) for side in ('low', 'high'))
            lo, hi = (None if v is _MISSING else v for v in (lo, hi))
            if (lo is None) != (hi is None):
                raise ValueError('--precursor_window_open_low and --precursor_window_open_high go together')
            if lo is not None:
                kw['precursor_window_open'] = (lo, hi)
        kw.update(overrides)
        if kw.get('index') is None:
            kw.pop('index', None)
        return cls(**kw)


def _lookup(obj, name):
    if obj is None:
        return _MISSING
    if isinstance(obj, dict):
        return obj.get(name, _MISSING)
    try:
        return getattr(obj, name)
    except (AttributeError, KeyError):
        return _MISSING


def add_arguments(parser) -> None:
    """The additive command-line flags, for the reference's parser: one call at the end of
    ``ann_solo.config.Config.__init__`` (config.py:268, before ``self._namespace = None`` at :270):

        from ann_solo_amd.config import add_arguments; add_arguments(self._parser)

    No existing flag changes name, default or meaning."""
    d = Config()
    parser.add_argument('--index', default=d.index, type=str, choices=['ivfflat', 'ivfpq', 'winflat'],
                        help='ANN index type: inverted file with exact inner products (the '
                             "reference's index) or with product-quantised codes, or 'winflat': exact inner "
                             "products over every library vector in the query's precursor window, no coarse "
                             'quantiser (--num_list and --num_probe are ignored; one GPU) '
                             '(default: %(default)s)')
    parser.add_argument('--pq_m', default=d.pq_m, type=int,
                        help='IVF-PQ: number of sub-quantisers; must divide hash_len '
                             '(default: %(default)s)')
    parser.add_argument('--pq_bits', default=d.pq_bits, type=int,
                        help='IVF-PQ: bits per sub-quantiser code (default: %(default)s)')
    parser.add_argument('--refine_k', default=d.refine_k, type=int,
                        help='IVF-PQ: re-rank this many ADC candidates with exact inner products '
                             '(default: no re-ranking)')
    parser.add_argument('--kmeans_niter', default=d.kmeans_niter, type=int,
                        help='k-means iterations when training the ANN index '
                             '(default: %(default)s)')
    parser.add_argument('--ann_seed', default=d.seed, type=int,
                        help='random seed of the ANN index trainer (default: %(default)s)')
    parser.add_argument('--flat_storage', default=d.flat_storage, type=str, choices=['fx22', 'fp32'],
                        help='IVF-Flat: store vector components as float32 (what FAISS stores) or, '
                             'opt-in, those in [0, 1) as 22-bit fixed point (4-byte postings, '
                             '|dx| <= 1.2e-7) (default: %(default)s)')
    parser.add_argument('--num_gpus', default=d.num_gpus, type=int,
                        help='shard the ANN index by inverted list over this many GPUs; the job '
                             'runs one process per GPU (torchrun --nproc-per-node N) and N must '
                             'equal this value; 0 or 1: every process searches the whole index '
                             '(default: %(default)s)')
    parser.add_argument('--ann_window', default=d.ann_window, type=str, choices=['post', 'pre'],
                        help="open search with the ANN index: 'post' keeps the k best vectors of the "
                             "probed lists, then those in the precursor window (the reference); 'pre' "
                             'keeps the k best vectors of the probed lists that are in the window '
                             '(IVF-PQ, m = 32, 8 bits; one GPU) (default: %(default)s)')
    parser.add_argument('--pq_by_residual', default=int(d.pq_by_residual), type=int, choices=[0, 1],
                        help="IVF-PQ: 1 quantises the residuals x - centroid (FAISS' IndexIVFPQ.by_residual); "
                             '0 the hashed vectors themselves, whose sparsity the centroid does not destroy '
                             '(needs --index ivfpq) (default: %(default)s)')
    parser.add_argument('--num_matches', default=d.num_matches, type=int,
                        help='library matches reported per query, best first (1 .. 16): above 1 every '
                             'SSM also carries its runners-up and the score gap to the second best; '
                             'identifications, scores and FDR are those of the best match; one GPU '
                             '(default: %(default)s)')
    parser.add_argument('--precursor_window_open_low', default=None, type=float,
                        help='open search: lowest neutral mass difference (query - library, Da; may be '
                             'negative) a candidate may have, instead of -precursor_tolerance_mass_open; '
                             'needs --precursor_window_open_high; one GPU (default: the symmetric window)')
    parser.add_argument('--precursor_window_open_high', default=None, type=float,
                        help='open search: highest neutral mass difference (query - library, Da) a '
                             'candidate may have; needs --precursor_window_open_low; one GPU '
                             '(default: the symmetric window)')
    parser.add_argument('--fragment_tolerance_unit', default=d.fragment_tolerance_unit, type=str,
                        choices=['Da', 'ppm'],
                        help="unit of --fragment_mz_tolerance in the (shifted) dot product: 'Da', one window "
                             "width for every peak (the reference), or 'ppm' of the query peak's m/z; not "
                             "the reference's --fragment_tol_mode, which only reaches its decoy annotation; "
                             'one GPU (default: %(default)s)')
    parser.add_argument('--distinct_matches', action='store_true', default=d.distinct_matches,
                        help='with --num_matches above 1: one rank per library peptide -- the '
                             "runners-up are the best matches of other peptides and the score gap is "
                             'the gap to the next different identification; one GPU '
                             '(default: every library spectrum is a rank of its own)')
    parser.add_argument('--score_stats', action='store_true', default=d.score_stats,
                        help='every SSM also carries n_scored, the candidates its query scored, and expect, '
                             "the number of them expected to reach the best match's score by chance (a "
                             "log-linear fit to the tail of the query's score histogram; a descriptive "
                             'statistic, not a calibrated p-value); identifications and scores do not change; '
                             'the batches run synchronously; one GPU (default: off)')
    parser.add_argument('--device_decoys', action='store_true', default=d.device_decoys,
                        help='add a shuffle-and-reposition decoy of every library spectrum, made on the GPU '
                             "while the library is read (not the reference's --add_decoys: leave that off); "
                             'the annotation tolerance is --fragment_mz_tolerance in --decoy_tolerance_unit, '
                             'the shuffle is keyed by --ann_seed (default: off)')
    parser.add_argument('--decoy_tolerance_unit', default=d.decoy_tolerance_unit, type=str,
                        choices=['ppm', 'Da'],
                        help="with --device_decoys: unit of --fragment_mz_tolerance in the fragment annotation "
                             "(the reference's --fragment_tol_mode) (default: %(default)s)")
    parser.add_argument('--localize_modifications', action='store_true', default=d.localize_modifications,
                        help='after the search, localise the precursor mass difference of every open-search '
                             'identification on its library peptide from the query spectrum (plain and shifted '
                             'b / y fragments within --fragment_mz_tolerance; ppm is of the theoretical m/z): '
                             'the SSMs gain mod_mass, mod_site_lo / _hi (0-based residues), mod_site_score, '
                             '_margin and _gain; identifications, scores and files do not change; one GPU '
                             '(default: off)')
    parser.add_argument('--device_fdr', action='store_true', default=d.device_fdr,
                        help="gate both cascade levels by the engine's own FDR step at --fdr: with --model none "
                             'target-decoy q-values on the cosine, with --model svm a Percolator-like linear SVM '
                             "over the reference's SSM features, trained on the GPU (--model rf needs --device_forest); "
                             'open-level q-values per mass-difference group of --fdr_min_group_size; one GPU '
                             '(default: off -- the caller scores the SSMs)')
    parser.add_argument('--device_forest', action='store_true', default=d.device_forest,
                        help="with --device_fdr and --model rf: the engine's histogram random forest, grown and "
                             'evaluated on the GPU -- binned splits (at most 256 bins per feature), depth at most '
                             "12, not scikit-learn's exact-split forest, hence a switch of its own; one GPU "
                             '(default: off -- --model rf is not provided)')
    parser.add_argument('--forest_trees', default=d.forest_trees, type=int,
                        help='with --device_forest: trees per forest (default: %(default)s)')
    parser.add_argument('--device_qvalues', action='store_true', default=d.device_qvalues,
                        help="with --device_fdr: the FDR step's target-decoy q-values (every relabelling round, the "
                             'held-out parts, the grouped step) by a radix sort and scans on the GPU instead of '
                             'numpy on the host; the same bytes either way; one GPU (default: off)')
    parser.add_argument('--device_groups', action='store_true', default=d.device_groups,
                        help="with --device_fdr: the open level's mass-difference groups (histogram peaks per nominal "
                             'mass difference) by integer histograms on the GPU instead of scipy on the host; the '
                             'same labels either way, and the scorer keeps the modification profile; one GPU '
                             '(default: off)')
    parser.add_argument('--chimeric_search', action='store_true', default=d.chimeric_search,
                        help='after the last cascade level, remove the peaks every accepted identification explains '
                             'from its query spectrum and search the residue once more (no peak shifts) among the '
                             "library spectra of the same charge inside the query's isolation window; a match of "
                             'another peptide is reported as a second PSM of the spectrum (chimeric_rank 1, '
                             'explained_intensity); one GPU (default: off)')
    parser.add_argument('--chimeric_window', default=d.chimeric_window, type=float,
                        help="with --chimeric_search: full width in m/z of the window around the query's precursor "
                             'when the queries carry no isolation_window (default: %(default)s)')
    parser.add_argument('--device_mgf', action='store_true', default=d.device_mgf,
                        help='read a query file whose name ends in .mgf with the GPU reader: lines, parameters and '
                             "numerals are parsed by kernels and the peaks never become Python objects; the same "
                             'queries as the host reader gives; malformed blocks raise an error naming the line or '
                             'spectrum; other query formats are read as before (default: off)')
    parser.add_argument('--device_mzml', action='store_true', default=d.device_mzml,
                        help='read a query file whose name ends in .mzML with the GPU reader: tags and parameters are '
                             'parsed and the base64 / zlib peak arrays decoded by kernels; the same queries as the '
                             'host reader gives; only MS2 spectra are read; malformed spectra raise an error naming '
                             'the spectrum; mzXML has a switch of its own, --device_mzxml (default: off)')
    parser.add_argument('--device_mzxml', action='store_true', default=d.device_mzxml,
                        help='read a query file whose name ends in .mzXML with the GPU reader: nested scans, precursor '
                             'text and ISO-8601 retention times are parsed and the interleaved big-endian base64 / '
                             'zlib peak streams decoded by kernels; the same queries as the host reader gives; only '
                             'MS2 scans are read; malformed scans raise an error naming the scan (default: off)')
    parser.add_argument('--device_library', action='store_true', default=d.device_library,
                        help='read a spectral library whose name ends in .sptxt with the GPU reader: records, '
                             'precursors, peaks and annotations are parsed by kernels, no reference package is '
                             'needed and no .spcfg / .hdf5 is written; the same packed store as the host reader '
                             'gives; malformed records raise an error naming the line or record; other library '
                             'formats are read as before (default: off)')
