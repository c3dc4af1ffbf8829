"""smmd_fid_trace_sqrt (the FID's spectral step as Newton-Schulz products on
v_mfma_f64_16x16x4_f64) on the MI355X against the float64 eigh path.

d = 1 and 130 take the edge masks, 130 more than one 128 x 128 block tile per
side, 48 less than one; d = 1 is odd and takes the scalar loads as well.

BOUND: a float64 numpy mirror of the iteration (delta = 1e-14, 52 iterations)
differed from the eigh value by at most 1.14e-6 of the traces over these kinds
(the shift's cost on singular covariances); x4 for the kernel's other summation
order.  RESIDUAL: the mirror's |Y^2 - Y0|_F stayed under 2e-9; 1e-6 is the
limit past which frechet_distance falls back to the host."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

BOUND = 5e-6
RESIDUAL = 1e-6
DIMS = [1, 48, 130]
KINDS = ['full', 'ill', 'rank']


@functools.lru_cache(maxsize=None)
def codes_for(d, kind, seed):
    """float32 codes: columns scaled by exp(-decay j / d) (decay 12 for 'ill',
    else 3), mixed by a random d x d matrix; 4 d rows, 'rank': max(2, d / 2)."""
    rng = np.random.default_rng(1000 * d + seed)
    n = max(2, d // 2) if kind == 'rank' else 4 * d
    x = rng.standard_normal((n, d)) * np.exp(-(12.0 if kind == 'ill' else 3.0) * np.arange(d) / d)
    return (x @ rng.standard_normal((d, d))).astype(np.float32)


def moments_for(dev, d, kind, seed):
    x = codes_for(d, kind, seed).astype(np.float64)
    cov = np.atleast_2d(np.cov(x, rowvar=False))
    return torch.from_numpy(x.mean(0)).to(dev), torch.from_numpy(cov).to(dev)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', DIMS)
def test_device_against_host(dev, d, kind, monkeypatch):
    from gan.core import fid
    mg, cg = moments_for(dev, d, kind, 1)
    mr, cr = moments_for(dev, d, kind, 2)
    # the ABI itself (no fallback behind it): both roots converged
    out4 = fid.trace_sqrt(cg, cr).tolist()
    print('d %d %s: tr_sqrt %.9e residuals %.3e %.3e c3 %.3e' % ((d, kind) + tuple(out4)))
    assert np.isfinite(out4).all()
    assert out4[1] <= RESIDUAL and out4[2] <= RESIDUAL
    monkeypatch.setattr(fid, '_warned', False)
    for tag, (m2, c2) in (('different sets', (mr, cr)), ('a set against itself', (mg, cg.clone()))):
        traces = float(torch.trace(cg) + torch.trace(c2))
        host = fid.frechet_distance(mg, cg, m2, c2, spectral='host')
        with warnings.catch_warnings():
            warnings.simplefilter('error')                 # a fallback would warn
            got = fid.frechet_distance(mg, cg, m2, c2, spectral='device')
        print('d %d %s, %s: device %.9e host %.9e, |diff| / traces %.3e'
              % (d, kind, tag, got, host, abs(got - host) / traces))
        assert abs(got - host) <= BOUND * traces


def test_deterministic_on_a_poisoned_workspace(dev):
    from gan.core import _lib
    d = 130
    _, cg = moments_for(dev, d, 'rank', 1)
    _, cr = moments_for(dev, d, 'rank', 2)
    L = _lib.lib()
    need = L.smmd_fid_trace_sqrt_workspace_bytes(d)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):                                     # poisoned, then as the call left it
        out4 = torch.empty(4, device=dev, dtype=torch.float64)
        _lib.check(L.smmd_fid_trace_sqrt(_lib.ptr(cg), _lib.ptr(cr), d, 1e-14, 52, _lib.ptr(out4),
                                         _lib.ptr(ws), ctypes.c_size_t(need),
                                         _lib.stream_handle(dev)), 'smmd_fid_trace_sqrt')
        outs.append(out4)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_fid_score_device(dev):
    from gan import compute_scores as cs
    G = torch.from_numpy(codes_for(130, 'full', 1)).to(dev)
    R = torch.from_numpy(codes_for(130, 'full', 2)).to(dev)
    host = cs.fid_score(G, R, splits=1, split_method='openai', spectral='host')
    got = cs.fid_score(G, R, splits=1, split_method='openai', spectral='device')
    traces = sum(np.trace(np.cov(t.cpu().numpy().astype(np.float64), rowvar=False)) for t in (G, R))
    print('fid_score device %.9e host %.9e, |diff| / traces %.3e'
          % (got[0], host[0], abs(got[0] - host[0]) / traces))
    assert got.shape == (1,) and abs(got[0] - host[0]) <= BOUND * traces
