"""BASELINE.json configs[0..1] as parity cases at their stated size (iPRG2012-scale library,
~9k spectra): config 0 = brute-force search on the CPU reference path (here: oracle) vs the
device window search; config 1 = IVF-Flat ANN + dot-product rescoring with the reference's
default index parameters (num_list 256, num_probe 128, num_candidates 1024)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def iprg(O):
    from ann_solo_amd import synthetic
    lib, aux = synthetic.make_library(9000, seed=20240807, device='cpu')
    return lib, aux


from oracle_backend import oracle_ivf as _oracle_ivf      # noqa: E402


def test_config0_bruteforce_cosine_plumbing(O, iprg):
    """--mode bf, standard 20 ppm search then open 300 Da search, no ANN: every query's
    winner, score and peak matches equal the CPU reference path (oracle)."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = iprg
    sl = SpectralLibrary(lib, config=Config.open_search(mode='bf'))
    for z in (2, 3):
        q, truth = synthetic.make_queries(lib, aux, 150, seed=100 + z, charge=z)
        part = sl.partitions[z]
        L = O.Spectra(*part.spectra.to('cpu').numpy())
        Q = O.Spectra(*q.numpy())
        for mode, tol, tmode in (('std', 20, 'ppm'), ('open', 300, 'Da')):
            res = sl._search_batch(q, z, mode)
            for i in range(q.n):
                d = np.abs(Q.precursor_mz[i] - part.precursor_mz.astype(np.float64))
                ok = d * z <= tol if tmode == 'Da' else d / part.precursor_mz.astype(np.float64) * 1e6 <= tol
                cand = np.nonzero(ok)[0]
                b, s, m = O.best_match(Q, i, L, cand, 0.02, True)
                assert res.n_candidates[i] == len(cand)
                if b < 0:
                    assert res.best_row[i] == -1
                else:
                    assert res.best_row[i] == cand[b] and res.best_score[i] == s
                    assert np.array_equal(res.peak_matches(i), m)
                    # reported cosine (spectrum_similarity.py:95-106) over the peak matches
                    qm, qi_, _ = Q.peaks(i)
                    lm, li, _ = L.peaks(int(cand[b]))
                    cos = float(np.dot(qi_[m[:, 0]], li[m[:, 1]])) if len(m) else 0.0
                    assert cos >= s - 1e-6
        # unmodified queries are found by the 20 ppm standard search
        res = sl._search_batch(q, z, 'std')
        rows = np.nonzero(lib.precursor_charge.numpy() == z)[0]
        unmod = ~truth['is_modified'].numpy()
        hit = rows[np.clip(res.best_row, 0, None)] == truth['source_row'].numpy()
        assert hit[unmod].mean() > 0.95


def test_config1_ivfflat_default_parameters(O, iprg):
    """IVF-Flat with the reference defaults, one batch per charge: ANN ids, winners, scores
    and peak matches identical to the oracle on the same index."""
    from ann_solo_amd import synthetic
    from ann_solo_amd.spectral_library import Config, SpectralLibrary
    lib, aux = iprg
    cfg = Config.open_search(index='ivfflat', kmeans_niter=10)       # num_list 256, num_probe 128, k 1024
    sl = SpectralLibrary(lib, config=cfg)
    assert sorted(sl._ann_filenames) == [2, 3, 4]
    for z in (2, 3, 4):
        q, truth = synthetic.make_queries(lib, aux, 200, seed=110 + z, charge=z)
        res = sl._search_batch(q, z, 'open', want_knn=True)
        part = sl.partitions[z]
        ref = O.search_batch(O.Spectra(*q.numpy()), O.Spectra(*part.spectra.to('cpu').numpy()),
                             part.precursor_mz, z, _oracle_ivf(O, part.index), 1024, 128, 300,
                             'Da', 0.02, True, pm_stride=res.pm_pairs.shape[1], want_knn=True)
        assert np.array_equal(res.knn, ref['knn_I'])
        assert np.array_equal(res.best_row, ref['best_row'])
        assert np.array_equal(res.best_score, ref['best_score'])
        assert np.array_equal(res.pm_count, ref['pm_count'])
        # the 10 exact nearest neighbours are (almost always) inside the ANN top-1024;
        # deeper ranks are near-orthogonal noise for hashed spectra (cf. the reference's
        # notebooks/iprg2012_num_candidates.ipynb), so recall@1024 itself is ~nprobe/nlist
        from ann_solo_amd import faiss_compat as faiss
        vec = sl._encode(part.spectra)
        flat = faiss.IndexFlatIP(800)
        flat.add(vec)
        _, Ie = flat.search(sl._encode(q.to('cuda')), 10)
        Ie = Ie.cpu().numpy()
        rec = np.mean([len(set(res.knn[i]) & set(Ie[i])) / 10 for i in range(q.n)])
        assert rec > 0.8, rec


def test_default_bench_line_at_small_size():
    """`python bench.py --full` at a size that takes seconds: every block the round-4
    line carries must be there and its parity flags true -- recall with the exact hit@k fields,
    the fixed-recall leg with its own roofline / parity / CPU baseline, the configs[4] cascade
    pass with oracle parity, the stage rates with the candidate count the kernel reports."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--library-size', '60000', '--nlist', '256',
           '--niter', '4', '--batch', '1024', '--steps', '2', '--warmup', '1', '--cpu-seconds', '2',
           '--recall-queries', '64', '--cascade-batches', '2', '--nprobe', '32', '--k', '256', '--full']
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    line = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert line, out.stderr[-3000:]
    d = json.loads(line[-1])
    assert d['metric'].startswith('query spectra/sec') and d['value'] > 0 and d['n_gpus'] == 1
    assert d['roofline']['bound'] == 'hbm' and d['roofline']['frac'] > 0 and d['dtype'] == 'f32'
    r = d['recall']
    assert 0 < r['exact_hit_at_k_source'] <= 1 and r['reference_exact_hit_at_1024_modified_iprg2012'] == 0.751
    cb = d['cpu_baseline']
    assert cb['value'] > 0 and cb['cores'] >= 1 and cb['parity_vs_gpu']['knn_id_sets_equal'] and \
        cb['parity_vs_gpu']['best_row_equal'] and cb['parity_vs_gpu']['best_score_max_abs_diff'] == 0.0
    f = d['fixed_recall']
    assert f['index'] == 'ivfflat' and f['value'] > 0 and f['storage'] == 'fp32'
    assert f['roofline']['layout'].startswith('float postings') and f['alt_storage']['storage'] == 'fx22'
    assert f['parity_vs_gpu']['knn_id_sets_equal'] and f['parity_vs_gpu']['best_row_equal']
    assert f['cpu_baseline']['dense_definition_check']['knn_ids_and_winners_equal'] is True
    c = d['cascade']
    assert c['value'] > 0 and c['levels']['std']['queries_in_per_step'] == 2048
    assert c['parity_vs_oracle']['all_equal'] is True and c['parity_vs_oracle']['queries'] >= 64
    g = d['stages_gbs']
    assert g['rescore']['candidate_count_equals_the_kernels'] is True and g['encode']['GBps'] > 0


@pytest.mark.parametrize('workload', ['batch', 'cascade'])
def test_plain_bench_line_and_dumped_outputs(tmp_path, workload):
    """`python bench.py` without --full: one line with the headline fields and none of the other legs;
    --dump-outputs writes what the last timed step returned, and two runs with the same arguments
    write the same arrays."""
    import glob
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n_batch, steps = 1024, 3

    def run(out_dir):
        cmd = [sys.executable, os.path.join(root, 'bench.py'), '--library-size', '60000', '--nlist', '256',
               '--niter', '4', '--batch', str(n_batch), '--steps', str(steps), '--warmup', '1', '--nprobe', '32',
               '--k', '256', '--workload', workload, '--dump-outputs', str(out_dir)]
        out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1 and lines[0].startswith('{'), (out.stdout[:500], out.stderr[-2000:])
        files = sorted(glob.glob(os.path.join(str(out_dir), '*.npy')))
        assert sum(os.path.getsize(f) for f in files) <= 64e6
        return json.loads(lines[0]), {os.path.basename(f)[:-4]: np.load(f) for f in files}
    d, a = run(tmp_path / 'a')
    assert d['metric'].startswith('query spectra/sec') and d['unit'] == 'query spectra/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f32' and d['steps'] == steps and d['n_gpus'] == 1
    assert d['value'] > 0 and d['ms_per_step'] > 0
    for leg in ('recall', 'fixed_recall', 'roofline', 'cpu_baseline', 'cascade', 'parity_vs_oracle',
                'device_stages_ms_per_step'):
        assert leg not in d, leg
    if workload == 'batch':
        nq = d['batch_per_step']
        # (ms_per_step is printed with 3 decimals: at a fraction of a millisecond per step its rounding, up to
        # 0.0005 ms, is more than 1e-3 of it -- the two figures agree to 1e-3 beyond what that rounding moves)
        assert d['value'] == pytest.approx(nq / (d['ms_per_step'] * 1e-3), rel=1e-3 + 0.0005 / d['ms_per_step'])
        assert set(a) == {'best_row', 'best_score', 'n_candidates', 'pm_count', 'pm_pairs'}
        assert all(a[k].shape == (nq,) and a[k].dtype == np.float64 for k in a if k != 'pm_pairs')
        assert a['pm_pairs'].dtype == np.float32 and a['pm_pairs'].shape[0] == nq
        assert (a['best_row'] >= -1).all() and (a['best_row'] < 60000).all() and (a['best_row'] >= 0).any()
    else:
        assert set(a) == {'qrow', 'lib_row', 'score', 'q'} and len(a['qrow']) == d['identifications']['total']
    _, b = run(tmp_path / 'b')
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
