"""mmd2_and_ratio on explicit matrices (the tuple path, plain torch ops) against
a float64 statement of gan/core/mmd.py:236-293, which the GPU tests share."""
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import smmd_oracle as O  # noqa: E402
from oracle.torch_kernels import kernel_xy  # noqa: E402

MIN_VAR = 1e-5


@functools.lru_cache(maxsize=None)
def ratio_reference(name, m, d, biased, min_var=MIN_VAR):
    """Inputs X ~ N(0, 1), Y ~ N(0.7, 1.3^2) [m, d] (fp32 values) and, in
    float64: the three matrices, mmd2 / var_est / ratio as the reference forms
    them -- row sums with the diagonal entry (the constant, where the kernel
    declares one) taken out, the diagonal kept in mmd2's numerators -- their
    autograd gradients, the largest of var_est's six terms,
    kappa = that / |var_est| and the float64 rounding noise of var_est."""
    rng = np.random.default_rng(zlib.crc32(repr((name, m, d)).encode()))
    X = rng.standard_normal((m, d)).astype(np.float32)
    Y = (0.7 + 1.3 * rng.standard_normal((m, d))).astype(np.float32)
    spec = O.kernel_spec(name)
    Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    Yt = torch.tensor(Y, dtype=torch.float64, requires_grad=True)
    Kxx, Kxy, Kyy = kernel_xy(spec, Xt, Xt), kernel_xy(spec, Xt, Yt), kernel_xy(spec, Yt, Yt)
    if spec.const_diag is None:
        dx, dy = torch.diagonal(Kxx), torch.diagonal(Kyy)
    else:
        dx = dy = torch.full((m,), float(spec.const_diag), dtype=torch.float64)
    a, b = Kxx.sum(1) - dx, Kyy.sum(1) - dy          # rows without "the" diagonal
    r, c = Kxy.sum(1), Kxy.sum(0)
    A, B, C = a.sum(), b.sum(), c.sum()
    qxx, qyy = (Kxx ** 2).sum() - (dx ** 2).sum(), (Kyy ** 2).sum() - (dy ** 2).sum()
    den = m * m if biased else m * (m - 1)
    mmd2 = (A + dx.sum()) / den + (B + dy.sum()) / den - 2 * C / m ** 2
    m1 = m - 1
    terms = [2 / (m ** 2 * m1 ** 2) * (2 * (a ** 2).sum() - qxx + 2 * (b ** 2).sum() - qyy),
             -(4 * m - 6) / (m ** 3 * m1 ** 3) * (A ** 2 + B ** 2),
             4 * (m - 2) / (m ** 3 * m1 ** 2) * ((r ** 2).sum() + (c ** 2).sum()),
             -4 * (m - 3) / (m ** 3 * m1 ** 2) * (Kxy ** 2).sum(),
             -(8 * m - 12) / (m ** 5 * m1) * C ** 2,
             8 / (m ** 3 * m1) * ((A + B) * C / m - (a * r).sum() - (b * c).sum())]
    var = sum(terms)
    ratio = mmd2 / torch.sqrt(torch.clamp(var, min=min_var))
    big = max(abs(t.item()) for t in terms)
    # The reference's own rounding: a Gaussian kernel's diagonal is exactly its
    # constant, but float64 leaves raw D2 = O(1e-14) there, so sum K_ii^2 - m c^2
    # is noise, not zero.  It is all of var_est where every off-diagonal value
    # underflows (rbf at d = 40: var_est = 2e-20).
    noise = 0.0
    if spec.kind == 'rbf':
        noise = 2 / (m ** 2 * m1 ** 2) * sum(
            abs(((torch.diagonal(K) ** 2).sum() - (dx ** 2).sum()).item()) for K in (Kxx, Kyy))
    ref = {'X': X, 'Y': Y, 'K': (Kxx.detach(), Kxy.detach(), Kyy.detach()),
           'const': False if spec.const_diag is None else spec.const_diag,
           'big': big, 'noise': noise, 'kappa': big / abs(var.item())}
    for key, val in (('mmd2', mmd2), ('var', var), ('ratio', ratio)):
        gx, gy = torch.autograd.grad(val, (Xt, Yt), retain_graph=True)
        ref[key] = val.item()
        ref['d' + key] = (gx.numpy(), gy.numpy())
    return ref


@pytest.mark.parametrize('name', ['rbf', 'mix_rq_1dot', 'distance', 'dot'])
@pytest.mark.parametrize('biased', [False, True])
def test_tuple_path_matches_reference(name, biased):
    from gan.core import mmd
    ref = ratio_reference(name, 23, 3, biased)
    Kxx, Kxy, Kyy = ref['K']
    got = mmd.mmd2_and_ratio((Kxx, Kxy, Kyy, ref['const']), biased=biased, min_var_est=MIN_VAR)
    assert len(got) == 3 and all(t.dim() == 0 for t in got)
    for g, key in zip(got, ('mmd2', 'ratio', 'var')):
        assert abs(g.item() - ref[key]) <= 1e-12 * max(1.0, abs(ref[key])), (key, g.item(), ref[key])
    m2, var = mmd._mmd2_and_variance(Kxx, Kxy, Kyy, ref['const'], biased)
    assert m2.item() == got[0].item() and var.item() == got[2].item()
