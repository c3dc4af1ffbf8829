"""GPU: mmd.mmd2_and_ratio's fused launches (smmd_mmd2_ratio_fwd / _bwd) against
the float64 reference of test_ratio_host.ratio_reference.

Tolerances (fp32 per-pair arithmetic against float64 on the same inputs):
  mmd2      |d| <= 1e-5 + 1e-4 |ref|                     (the parity tests' _close)
  var_est   |d| <= 1e-4 * the largest of its six terms   (each carries the per-pair error)
            + the reference's own float64 rounding (ratio_reference's `noise`)
  ratio     rtol 1e-4 + 0.5e-4 kappa,  kappa = largest term / |var_est|
  gradients |d| <= 1e-4 s max|ref| + 1e-3 |ref|, s = max(1, kappa) for var_est and ratio
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_ratio_host import MIN_VAR, ratio_reference  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_SHAPES = [(5, 1), (64, 3), (130, 8)]          # d <= 8: below, at, across the row tile
MFMA_SHAPES = [(65, 9), (200, 16), (130, 40)]      # unpadded / padded K, several tiles a side
KERNELS = ['rbf', 'mix_rq_1dot', 'distance', 'dot']
# (kernel, (m, d), biased, SMMD_RATIO_CHUNKS): the last two cases run several
# column tiles per block on the MFMA path, and its two accumulators per
# weighting (d > 64)
CASES = ([(k, s, False, None) for k in KERNELS for s in TILE_SHAPES + MFMA_SHAPES]
         + [(k, s, True, None) for k in KERNELS for s in ((130, 8), (200, 16))]
         + [('mix_rq_1dot', (200, 16), False, '1'), ('mix_rq_1dot', (65, 72), False, None)])


def _run(dev, name, shape, biased, grads=True):
    from gan.core import mmd
    ref = ratio_reference(name, shape[0], shape[1], biased)
    assert not 0.5 * MIN_VAR <= ref['var'] <= 2 * MIN_VAR, 'the case sits on the clamp'
    X = torch.tensor(ref['X'], device=dev, requires_grad=grads)
    Y = torch.tensor(ref['Y'], device=dev, requires_grad=grads)
    out = mmd.mmd2_and_ratio(mmd.get_kernel(name)(X, Y), biased=biased, min_var_est=MIN_VAR)
    return ref, X, Y, out


def _check_values(ref, out, what):
    m2, ratio, var = (t.item() for t in out)
    print('%s: mmd2 %.3e var %.3e ratio %.3e kappa %.1f' % (
        what, m2 - ref['mmd2'], var - ref['var'], ratio - ref['ratio'], ref['kappa']))
    assert abs(m2 - ref['mmd2']) <= 1e-5 + 1e-4 * abs(ref['mmd2']), (what, m2, ref['mmd2'])
    assert abs(var - ref['var']) <= 1e-4 * ref['big'] + ref['noise'], (what, var, ref['var'])
    clamped = ref['var'] < MIN_VAR
    rtol = 1e-4 + (0.0 if clamped else 0.5e-4 * ref['kappa'])
    assert abs(ratio - ref['ratio']) <= rtol * abs(ref['ratio']), (what, ratio, ref['ratio'])


@pytest.mark.parametrize('name,shape,biased,chunks', CASES)
def test_values_and_gradients(dev, monkeypatch, name, shape, biased, chunks):
    if chunks:
        monkeypatch.setenv('SMMD_RATIO_CHUNKS', chunks)
    ref, X, Y, out = _run(dev, name, shape, biased)
    what = '%s %s biased=%s' % (name, shape, biased)
    _check_values(ref, out, what)
    clamped = ref['var'] < MIN_VAR
    for i, key in enumerate(('mmd2', 'ratio', 'var')):
        gx, gy = torch.autograd.grad(out[i], (X, Y), retain_graph=True)
        s = 1.0 if key == 'mmd2' or (key == 'ratio' and clamped) else max(1.0, ref['kappa'])
        for got, want in zip((gx, gy), ref['d' + key]):
            lim = 1e-4 * s * max(np.abs(want).max(), 1e-12) + 1e-3 * np.abs(want)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            print('%s d%s: max err %.3e of max|ref| %.3e' % (what, key, err.max(),
                                                             np.abs(want).max()))
            assert (err <= lim).all(), (what, key, err.max(), np.abs(want).max())


@pytest.mark.parametrize('shape', [(130, 8), (200, 16)])
def test_mix_rbf_values(dev, shape):
    ref, _, _, out = _run(dev, 'mix_rbf', shape, False, grads=False)
    _check_values(ref, out, 'mix_rbf %s' % (shape,))


@pytest.mark.parametrize('shape', [(200, 16), (130, 40)])
def test_clamped_ratio_gradient(dev, shape):
    """var_est < min_var_est: d ratio = d mmd2 / sqrt(min_var_est), and the
    third output still carries var_est's own gradient."""
    ref, X, Y, out = _run(dev, 'rbf', shape, False)
    assert ref['var'] < 0.5 * MIN_VAR
    gm = torch.autograd.grad(out[0], (X, Y), retain_graph=True)
    gr = torch.autograd.grad(out[1], (X, Y), retain_graph=True)
    gv = torch.autograd.grad(out[2], (X, Y))
    for a, b, v, want in zip(gm, gr, gv, ref['dvar']):
        assert torch.allclose(b, a / MIN_VAR ** 0.5, rtol=1e-6, atol=0)
        assert np.abs(want).max() > 0 and v.abs().max().item() > 0


@pytest.mark.parametrize('shape', [(130, 8), (200, 16)])
def test_deterministic_and_workspace_zero(dev, shape):
    from gan.core import _lib
    runs = []
    for _ in range(2):
        _, X, Y, out = _run(dev, 'mix_rq_1dot', shape, False)
        (out[1] + out[2]).backward()
        runs.append([t.detach().clone() for t in out] + [X.grad, Y.grad])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    ws = [buf for key, buf in _lib._ws_cache.items() if key[2] == 'mmd2_ratio']
    assert ws and all(not buf.any().item() for buf in ws)


def test_fused_switch_and_bad_input(dev, monkeypatch):
    from gan.core import mmd
    ref, X, Y, fused = _run(dev, 'mix_rq_1dot', (130, 8), False)
    monkeypatch.setenv('SMMD_RATIO_FUSED', '0')
    _, _, _, plain = _run(dev, 'mix_rq_1dot', (130, 8), False)
    _check_values(ref, plain, 'materialised')          # both sit within the reference's bounds
    for a, b in zip(fused, plain):
        assert torch.allclose(a, b, rtol=2e-4 * max(1.0, ref['kappa']), atol=2e-5)
    monkeypatch.delenv('SMMD_RATIO_FUSED')
    with pytest.raises(ValueError):
        mmd.mmd2_and_ratio(mmd._rbf_kernel(X, Y[:-1]))
