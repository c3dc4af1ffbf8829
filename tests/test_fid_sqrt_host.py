"""smmd_fid_trace_sqrt without a GPU: the library's argument and workspace
checks, the workspace's closed form, and the opt-in switch of
frechet_distance."""
import ctypes

import pytest

torch = pytest.importorskip('torch')


def test_library_argument_checks():
    from gan.core import _lib
    L = _lib.lib()
    x = ctypes.c_void_p(4096)
    # every call below is refused before any launch (x is not a real buffer)
    def call(g=x, r=x, dim=70, delta=1e-14, iters=52, out=x, ws=x, nbytes=1 << 40):
        return L.smmd_fid_trace_sqrt(g, r, dim, delta, iters, out, ws, nbytes, None)
    assert call(g=None) == 1 and call(r=None) == 1 and call(out=None) == 1
    assert call(dim=0) == 1 and call(iters=0) == 1
    assert call(delta=0.0) == 1 and call(delta=-1e-14) == 1 and call(delta=float('nan')) == 1
    need = L.smmd_fid_trace_sqrt_workspace_bytes(70)
    assert call(ws=None) == 3 and call(nbytes=need - 1) == 3


def test_workspace_closed_form():
    from gan.core import _lib
    L = _lib.lib()
    assert L.smmd_fid_trace_sqrt_workspace_bytes(0) == 0
    assert L.smmd_fid_trace_sqrt_workspace_bytes(-3) == 0
    # the scalars, three partial slabs of one double per 128 x 128 tile, six
    # d x d double buffers (Y, Z, T, Y', Z', M), each rounded up to 256 bytes
    assert L.smmd_fid_trace_sqrt_workspace_bytes(2048) == 256 + 3 * 16 * 16 * 8 + 6 * 2048 * 2048 * 8
    assert L.smmd_fid_trace_sqrt_workspace_bytes(1) == 256 + 3 * 256 + 6 * 256


def test_device_switch_on_cpu_tensors(monkeypatch):
    from gan.core import _lib, fid
    mean = torch.zeros(3, dtype=torch.float64)
    cov = torch.eye(3, dtype=torch.float64)
    with pytest.raises(_lib.SmmdError):
        fid.frechet_distance(mean, cov, mean, cov, spectral='device')
    monkeypatch.setenv('SMMD_FID_SQRT', '1')                  # None reads the switch
    with pytest.raises(_lib.SmmdError):
        fid.frechet_distance(mean, cov, mean, cov)
    monkeypatch.setenv('SMMD_FID_SQRT', '0')
    assert abs(fid.frechet_distance(mean, cov, mean, cov)) <= 1e-12
    assert abs(fid.frechet_distance(mean, cov, mean, cov, spectral='host')) <= 1e-12
    with pytest.raises(ValueError):
        fid.frechet_distance(mean, cov, mean, cov, spectral='gpu')
    assert fid.sqrt_iters(1e-14) == 52


def test_flags():
    from gan import compute_scores as cs
    from gan.main import build_parser, default_flags
    from gan.utils.scorer import Scorer
    assert default_flags()['fid_spectral'] == 'host'
    assert build_parser().parse_args(['-fid_spectral', 'device']).fid_spectral == 'device'
    with pytest.raises(ValueError):
        Scorer(torch.zeros(4, 2).numpy(), fid=True, fid_spectral='gpu')
    with pytest.raises(SystemExit):
        cs.main(['g.npy', '--reference-feats', 'r.npy', '--fid-spectral', 'gpu'])
