"""smmd_code_moments and the FID on the MI355X against float64 numpy / scipy
on the same float32 codes.

The covariance and FID bounds are 4x the largest error measured on the GPU over
the shapes below (profiles/fid/fid_ab_*.json, "test_errors": rounding is
data-dependent, hence the margin), and stay under 2e-6, the bound of the
project's f32-MFMA parity tests."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

# max |cov - cov64| / max |cov64|: measured 0 .. 1.956e-7 over SHAPES x (index None,
# bootstrap) and the offset case (the largest: (64, 64), index None)
COV_BOUND = 4 * 1.956e-7
# |fid - reference| / reference on the three host-test inputs and the bootstrap
# case: measured 2.1e-9 .. 1.81e-8; identical sets: 5.6e-16 of the traces
FID_BOUND = 4 * 1.81e-8
assert COV_BOUND <= 2e-6 and FID_BOUND <= 2e-6

SHAPES = [(2, 1), (33, 5), (64, 64), (257, 96), (1500, 200), (300, 2048),
          (700, 70)]        # the last: a 512-row slice and a shorter one, two column tiles


def codes_for(n, d, offset=0.0):
    rng = np.random.default_rng(1000 * n + d)
    x = np.maximum(rng.standard_normal((n + 7, d)) + 0.5, 0.0) + offset
    return x.astype(np.float32)


def check_moments(dev, x, index, tag):
    from gan.core.fid import code_moments
    part = x.astype(np.float64) if index is None else x.astype(np.float64)[index]
    X = torch.from_numpy(x).to(dev)
    I = None if index is None else torch.from_numpy(index).to(dev)
    mean, cov = code_moments(X, I)
    assert mean.is_cuda and mean.dtype == cov.dtype == torch.float64
    rm = part.mean(0)
    rc = np.atleast_2d(np.cov(part, rowvar=False))
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    err_m = np.abs(mean - rm).max() / max(np.abs(rm).max(), 1e-300)
    err_c = np.abs(cov - rc).max() / max(np.abs(rc).max(), 1e-300)
    print('code_moments %s: mean err %.3e cov err %.3e' % (tag, err_m, err_c))
    assert err_m <= 1e-12
    assert np.array_equal(cov, cov.T)
    assert err_c <= COV_BOUND
    return err_c


@pytest.mark.parametrize('n,d', SHAPES)
def test_code_moments_all_rows(dev, n, d):
    x = codes_for(n, d)[:n]
    check_moments(dev, x, None, '(%d, %d) index None' % (n, d))
    # a view of the leading rows of a larger array (n < n_rows)
    from gan.core.fid import code_moments
    X = torch.from_numpy(codes_for(n, d)).to(dev)
    a = code_moments(X[:n])
    b = code_moments(torch.from_numpy(x).to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('n,d', SHAPES)
def test_code_moments_bootstrap_index(dev, n, d):
    x = codes_for(n, d)                                   # n_rows = n + 7
    index = np.random.default_rng(n + d).integers(0, n + 7, n).astype(np.int64)
    index[-1] = index[0]                                  # a repeat for sure
    check_moments(dev, x, index, '(%d, %d) bootstrap' % (n, d))


def test_code_moments_large_offset(dev):
    """Codes near +1000: without the shift the f32 products would lose the
    covariance altogether."""
    x = codes_for(257, 96, offset=1000.0)
    index = np.random.default_rng(9).integers(0, 264, 257).astype(np.int64)
    check_moments(dev, x[:257], None, '(257, 96) + 1000, index None')
    check_moments(dev, x, index, '(257, 96) + 1000, bootstrap')


def test_bad_index_raises(dev):
    from gan.core.fid import code_moments
    X = torch.from_numpy(codes_for(33, 5)).to(dev)
    for bad in ([0, 40], [-1, 2]):
        with pytest.raises(ValueError):
            code_moments(X, torch.tensor(bad, device=dev))


def test_deterministic_and_workspace_at_rest(dev):
    """Two calls on one workspace give the same bits and leave the same bytes
    in it; what it held before does not change the results (it carries no
    counters, and nothing is read before the call has written it)."""
    import ctypes
    from gan.core import _lib
    n, d = 1500, 200
    x = torch.from_numpy(codes_for(n, d)).to(dev)
    index = torch.from_numpy(np.random.default_rng(4).integers(0, n + 7, n)).to(dev)
    L = _lib.lib()
    need = L.smmd_code_moments_workspace_bytes(n, d)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    results, rests = [], []
    for fill in (None, None, 0xFF):
        if fill is not None:
            ws.fill_(fill)
        mean = torch.empty(d, device=dev, dtype=torch.float64)
        cov = torch.empty(d, d, device=dev, dtype=torch.float64)
        _lib.check(L.smmd_code_moments(_lib.ptr(x), n + 7, d, _lib.ptr(index), n, _lib.ptr(mean),
                                       _lib.ptr(cov), _lib.ptr(ws), ctypes.c_size_t(need),
                                       _lib.stream_handle(dev)), 'smmd_code_moments')
        results.append((mean, cov))
        rests.append(ws.clone())
    for mean, cov in results[1:]:
        assert torch.equal(mean, results[0][0]) and torch.equal(cov, results[0][1])
    assert torch.equal(rests[0], rests[1])


def test_switch_agrees_with_library(dev, monkeypatch):
    from gan.core.fid import code_moments
    n, d = 1500, 200
    x = torch.from_numpy(codes_for(n, d)).to(dev)
    index = torch.from_numpy(np.random.default_rng(4).integers(0, n + 7, n)).to(dev)
    mean, cov = code_moments(x, index)
    monkeypatch.setenv('SMMD_FID_COV', '0')
    mean0, cov0 = code_moments(x, index)
    assert mean0.is_cuda and cov0.dtype == torch.float64
    assert not torch.equal(cov, cov0)                     # another path did run
    err = float((cov - cov0).abs().max() / cov0.abs().max())
    print('library vs SMMD_FID_COV=0: cov err %.3e' % err)
    assert err <= COV_BOUND
    assert float((mean - mean0).abs().max()) <= 1e-12 * float(mean0.abs().max())


@pytest.fixture(scope='module')
def fid_references():
    """The host-test inputs and their float64 scipy scores on the whole sets,
    computed once."""
    import test_fid_host as H
    out = []
    for n, d, zeroed in H.CASES:
        g = H.make_codes(n, d, zeroed, 0.5)
        r = H.make_codes(n, d, zeroed, 0.4, seed_offset=1)
        score, ok = H.ref_fid_parts(g, r)
        assert ok
        out.append((g, r, score))
    return out


def test_fid_score_on_device(dev, fid_references):
    from gan import compute_scores as cs
    for g, r, want in fid_references:
        G, R = torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev)
        got = cs.fid_score(G, R, splits=1, split_method='openai')
        rel = abs(got[0] - want) / abs(want)
        print('fid_score %s: %.9f reference %.9f rel %.3e' % (g.shape, got[0], want, rel))
        assert rel <= FID_BOUND
        # numpy arrays go to the device too and give the same bits
        assert np.array_equal(cs.fid_score(g, r, splits=1, split_method='openai'), got)
        # the same codes on both sides: zero up to the bound on the traces
        same = cs.fid_score(G, G.clone(), splits=1, split_method='openai')
        tr = 2 * np.trace(np.cov(g.astype(np.float64), rowvar=False))
        print('fid_score %s identical sets: %.3e (traces %.3e)' % (g.shape, same[0], tr))
        assert abs(same[0]) <= FID_BOUND * tr


def test_fid_score_bootstrap_on_device(dev, fid_references):
    """Bootstrap splits draw the reference's indices and stay within the bound
    of the float64 path on the same draws."""
    from gan import compute_scores as cs
    g, r, _ = fid_references[1]
    np.random.seed(3)
    got = cs.fid_score(torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev), splits=2,
                       split_method='bootstrap')
    np.random.seed(3)
    want = cs.fid_score(torch.from_numpy(g), torch.from_numpy(r), splits=2,
                        split_method='bootstrap')
    rel = np.abs(got - want) / np.abs(want)
    print('fid_score bootstrap: rel', rel)
    assert np.all(rel <= FID_BOUND)


def test_cli_with_mmd(dev, tmp_path, capsys):
    from gan import compute_scores as cs
    rng = np.random.default_rng(0)
    np.save(tmp_path / 'g.npy', np.maximum(rng.standard_normal((300, 64)), 0).astype(np.float32))
    np.save(tmp_path / 'r.npy', np.maximum(rng.standard_normal((280, 64)) + 0.1, 0)
            .astype(np.float32))
    out = tmp_path / 'scores.npz'
    np.random.seed(0)
    assert cs.main([str(tmp_path / 'g.npy'), '--reference-feats', str(tmp_path / 'r.npy'),
                    '--do-fid', '--do-mmd', '--splits', '2', '--mmd-subsets', '3',
                    '--mmd-subset-size', '100', '--output', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'FID mean:' in text and 'KID mean:' in text
    saved = np.load(out)
    assert saved['fid'].shape == (2,) and saved['mmd2'].shape == (3,)
    assert np.isfinite(saved['fid']).all() and np.isfinite(saved['mmd2']).all()
