"""FID scoring without a GPU: the splits, fid_score and code_moments on CPU
tensors (their float64 path) against the reference formula restated here
(gan/compute_scores.py:159-208: np.cov and scipy.linalg.sqrtm), the library's
argument checks, the Scorer's opt-in FID block, the flag and the command line."""
import argparse
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

CASES = [(96, 32, 0), (200, 64, 3), (130, 96, 5)]       # (n, d, zeroed columns)


def make_codes(n, d, zeroed, b, seed_offset=0):
    """relu(N(0,1)[n, d] @ A + b) as float32, A = N(0,1)[d, d] / sqrt(d) from
    default_rng(0) (the same A on both sides), the first `zeroed` columns 0."""
    A = np.random.default_rng(0).standard_normal((d, d)) / np.sqrt(d)
    z = np.random.default_rng(1 + seed_offset).standard_normal((n, d))
    x = np.maximum(z @ A + b, 0.0).astype(np.float32)
    x[:, :zeroed] = 0.0
    return x


def ref_fid_parts(part_g, part_r):
    """The reference's per-split score (:193-206) in float64, and whether its
    first sqrtm was finite and real."""
    from scipy import linalg
    part_g, part_r = part_g.astype(np.float64), part_r.astype(np.float64)
    mn_g, mn_r = part_g.mean(axis=0), part_r.mean(axis=0)
    cov_g, cov_r = np.cov(part_g, rowvar=False), np.cov(part_r, rowvar=False)
    covmean, _ = linalg.sqrtm(cov_g.dot(cov_r), disp=False)
    ok = bool(np.isfinite(covmean).all()) and float(np.abs(np.imag(covmean)).max()) == 0.0
    score = np.sum((mn_g - mn_r) ** 2) + (np.trace(cov_g) + np.trace(cov_r)
                                          - 2 * np.trace(np.real(covmean)))
    return score, ok


def ref_fid_score(codes_g, codes_r, seed, **split_args):
    from gan import compute_scores as cs
    np.random.seed(seed)
    sg = cs.get_splits(len(codes_g), **split_args)
    sr = cs.get_splits(len(codes_r), **split_args)
    out = [ref_fid_parts(codes_g[a], codes_r[b]) for a, b in zip(sg, sr)]
    assert all(ok for _, ok in out), 'the reference sqrtm is not real and finite here'
    return np.array([s for s, _ in out])


def test_get_splits():
    from gan import compute_scores as cs
    assert cs.get_splits(10, splits=3, split_method='openai') == [slice(0, 3), slice(3, 6),
                                                                  slice(6, 10)]
    assert cs.get_splits(10, splits=3) == cs.get_splits(10, splits=3, split_method='openai')
    np.random.seed(0)
    got = cs.get_splits(7, splits=2, split_method='bootstrap')
    np.random.seed(0)
    want = [np.random.choice(7, 7), np.random.choice(7, 7)]
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        cs.get_splits(10, splits=3, split_method='nope')


# Both split methods.  One openai split is the whole set.  A bootstrap draw of n
# rows keeps about 0.63 n distinct ones, so (130, 96) resampled has fewer
# distinct rows than non-zero columns and the reference's sqrtm turns complex
# there (asserted in ref_fid_score): that case runs on the whole set only.
@pytest.mark.parametrize('n,d,zeroed,method', [c + ('openai',) for c in CASES]
                         + [c + ('bootstrap',) for c in CASES[:2]])
def test_fid_score_cpu_matches_reference(n, d, zeroed, method):
    from gan import compute_scores as cs
    g, r = make_codes(n, d, zeroed, 0.5), make_codes(n, d, zeroed, 0.4, seed_offset=1)
    split_args = dict(splits=1 if method == 'openai' else 2, split_method=method)
    want = ref_fid_score(g, r, 5, **split_args)
    np.random.seed(5)
    got = cs.fid_score(torch.from_numpy(g), torch.from_numpy(r), **split_args)
    assert isinstance(got, np.ndarray) and got.shape == want.shape
    print('fid', got, 'reference', want, 'rel', np.abs(got - want) / np.abs(want))
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want))


def test_fid_score_fewer_rows_than_columns():
    """n < d: the reference may take its eps path, so the check is against the
    eigenvalue formula in numpy float64; the score is finite and not negative
    beyond rounding."""
    from gan import compute_scores as cs
    g, r = make_codes(40, 64, 0, 0.5), make_codes(40, 64, 0, 0.4, seed_offset=1)
    got = cs.fid_score(torch.from_numpy(g), torch.from_numpy(r), splits=1, split_method='openai')
    g64, r64 = g.astype(np.float64), r.astype(np.float64)
    cg, cr = np.cov(g64, rowvar=False), np.cov(r64, rowvar=False)
    w, V = np.linalg.eigh(cg)
    s = (V * np.sqrt(np.maximum(w, 0))) @ V.T
    M = s @ cr @ s
    lam = np.linalg.eigvalsh((M + M.T) / 2)
    want = (np.sum((g64.mean(0) - r64.mean(0)) ** 2) + np.trace(cg) + np.trace(cr)
            - 2 * np.sqrt(np.maximum(lam, 0)).sum())
    assert np.isfinite(got).all()
    # M has d - n + 1 = 25 null eigenvalues; each comes out of eigvalsh as
    # +-eps |M| and its clamped square root as up to sqrt(eps |M|), in both
    # evaluations, and the trace term counts twice
    tol = 2 * 2 * 25 * np.sqrt(np.finfo(np.float64).eps * np.abs(lam).max())
    print('n < d: got', got[0], 'eigen formula', want, 'tol', tol)
    assert abs(got[0] - want) <= tol + 1e-9 * abs(want)
    assert got[0] >= -1e-9 * (np.trace(cg) + np.trace(cr))


def test_code_moments_cpu():
    from gan.core.fid import code_moments
    x = make_codes(130, 96, 5, 0.5)
    idx = np.random.default_rng(3).integers(0, 130, 90)
    idx[:4] = idx[4:8]                                   # repeated rows for sure
    for index in (None, idx):
        part = x.astype(np.float64) if index is None else x.astype(np.float64)[index]
        mean, cov = code_moments(torch.from_numpy(x),
                                 None if index is None else torch.from_numpy(index))
        assert mean.dtype == cov.dtype == torch.float64 and cov.shape == (96, 96)
        rm, rc = part.mean(0), np.cov(part, rowvar=False)
        assert np.abs(mean.numpy() - rm).max() <= 1e-12 * np.abs(rm).max()
        assert np.abs(cov.numpy() - rc).max() <= 1e-12 * np.abs(rc).max()
        assert torch.equal(cov, cov.t())
    for bad in ([0, 130], [-1, 3]):
        with pytest.raises(ValueError):
            code_moments(torch.from_numpy(x), torch.tensor(bad))


def test_library_argument_checks():
    from gan.core import _lib
    L = _lib.lib()
    x = ctypes.c_void_p(4096)
    # every call below is refused before any launch (x is not a real buffer)
    assert L.smmd_code_moments_workspace_bytes(0, 8) == 0
    assert L.smmd_code_moments_workspace_bytes(1, 8) == 0
    assert L.smmd_code_moments_workspace_bytes(8, 0) == 0
    need = L.smmd_code_moments_workspace_bytes(100, 70)
    assert need >= 3 * 64 * 64 * 8                       # 3 tiles on or above the diagonal
    big = 1 << 30
    assert L.smmd_code_moments(None, 100, 70, x, 100, x, x, x, big, None) == 1
    assert L.smmd_code_moments(x, 100, 70, x, 100, None, x, x, big, None) == 1
    assert L.smmd_code_moments(x, 100, 70, x, 100, x, None, x, big, None) == 1
    assert L.smmd_code_moments(x, 100, 70, x, 1, x, x, x, big, None) == 1       # n < 2
    assert L.smmd_code_moments(x, 100, 0, x, 100, x, x, x, big, None) == 1      # dim < 1
    assert L.smmd_code_moments(x, 0, 70, x, 100, x, x, x, big, None) == 1       # no rows
    assert L.smmd_code_moments(x, 100, 70, None, 101, x, x, x, big, None) == 1  # n > n_rows
    assert L.smmd_code_moments(x, 100, 70, None, 100, x, x, None, big, None) == 3
    assert L.smmd_code_moments(x, 100, 70, None, 100, x, x, x, need - 1, None) == 3
    assert L.smmd_code_moments(x, 100, 70, x, 100, x, x, x, need - 1, None) == 3
    # the scorer's shape: about 1024 blocks, a workspace of a few tens of MB
    full = L.smmd_code_moments_workspace_bytes(25000, 2048)
    assert 528 * 64 * 64 * 8 <= full <= 48 << 20


class _Gan:
    config = argparse.Namespace(MMD_sdlr_freq=1, MMD_sdlr_past_sample=2, MMD_sdlr_num_test=3,
                                with_scaling=False)
    lr = 1e-4

    def __init__(self, timer=True):
        self.lines = []
        if timer:
            self.timer = lambda step, mess='': self.lines.append((step, mess))

    def decay_ops(self):
        pass


def _patch_scoring(monkeypatch, calls):
    from gan.utils import scorer as S

    def fake_fid(codes_g, codes_r, **kw):
        calls.append(('fid', kw))
        return np.array([3.0, 5.0, 4.0])

    def fake_kid(*a, **k):
        calls.append(('kid', k))
        np.random.random()                              # the KID draws from the global stream
        return np.full(2, 0.5)
    monkeypatch.setattr(S.cs, 'fid_score', fake_fid)
    monkeypatch.setattr(S.cs, 'polynomial_mmd_averages', fake_kid)
    monkeypatch.setattr(S.mmd, 'np_diff_polynomial_mmd2_and_ratio_with_saving',
                        lambda X, Y, saved: ('sums',))
    return S


def test_scorer_with_fid(monkeypatch):
    calls = []
    S = _patch_scoring(monkeypatch, calls)
    gan = _Gan()
    sc = S.Scorer(np.zeros((10, 4)), n_subsets=2, subset_size=5, fid=True)
    out = sc.compute(gan, 0, np.zeros((10, 4)))
    assert [c[0] for c in calls] == ['fid', 'kid']                 # the reference's order
    assert calls[0][1] == dict(split_method='bootstrap', splits=3)
    assert np.array_equal(out['fid'], [3.0, 5.0, 4.0]) and 'mmd2' in out
    want = "FID mean (std): %f (%f)" % (4.0, np.std([3.0, 5.0, 4.0]))
    assert (0, want) in gan.lines
    # other split count, and a gan without a timer
    calls.clear()
    out = S.Scorer(np.zeros((10, 4)), n_subsets=2, subset_size=5, fid=True,
                   fid_splits=5).compute(_Gan(timer=False), 0, np.zeros((10, 4)))
    assert calls[0][1]['splits'] == 5 and 'fid' in out


def test_scorer_default_is_unchanged(monkeypatch):
    calls = []
    S = _patch_scoring(monkeypatch, calls)

    def parent_compute(codes, train):
        """Scorer.compute as it was before the FID block (first scoring, lr
        scheduler on): the KID, then the 3-sample sums."""
        out = {'mmd2': S.cs.polynomial_mmd_averages(codes, train, n_subsets=2, subset_size=5,
                                                    ret_var=False)}
        S.mmd.np_diff_polynomial_mmd2_and_ratio_with_saving(train[:2048], codes[:2048], None)
        return out

    np.random.seed(11)
    gan = _Gan()
    out = S.Scorer(np.zeros((10, 4)), n_subsets=2, subset_size=5).compute(gan, 0,
                                                                          np.zeros((10, 4)))
    after = np.random.random()
    assert [c[0] for c in calls] == ['kid'] and 'fid' not in out
    assert not any('FID' in m for _, m in gan.lines)
    np.random.seed(11)
    parent_compute(np.zeros((10, 4)), np.zeros((10, 4), dtype=np.float32))
    assert np.random.random() == after


def test_compute_fid_flag():
    from gan.main import build_parser, default_flags
    assert default_flags()['compute_fid'] is False
    assert build_parser().parse_args(['-compute_fid', 'true']).compute_fid is True


def test_cli_on_cpu(tmp_path, capsys):
    from gan import compute_scores as cs
    g, r = make_codes(96, 32, 0, 0.5), make_codes(80, 32, 0, 0.4, seed_offset=1)
    np.save(tmp_path / 'g.npy', g)
    np.save(tmp_path / 'r.npy', r)
    out = tmp_path / 'sub' / 'scores.npz'
    np.random.seed(2)
    rc = cs.main([str(tmp_path / 'g.npy'), '--reference-feats', str(tmp_path / 'r.npy'),
                  '--do-fid', '--no-mmd', '--splits', '2', '--split-method', 'bootstrap',
                  '--device', 'cpu', '--output', str(out)])
    assert rc == 0
    text = capsys.readouterr().out
    assert 'FID mean:' in text and 'FID std:' in text
    saved = np.load(out)
    assert saved.files == ['fid'] and saved['fid'].shape == (2,)
    np.random.seed(2)
    want = cs.fid_score(torch.from_numpy(g), torch.from_numpy(r), splits=2,
                        split_method='bootstrap')
    assert np.array_equal(saved['fid'], want)
    with pytest.raises(SystemExit):                       # an existing output is not overwritten
        cs.main([str(tmp_path / 'g.npy'), '--reference-feats', str(tmp_path / 'r.npy'),
                 '--device', 'cpu', '--output', str(out)])
