"""oracle/torch_kernels.py (the float64 autograd restatement of the kernel
family) against the numpy oracle: values to 1e-12, the autograd first order
against the oracle's analytic gradients to 1e-10, and the second order against
central differences of the oracle's witness gradient at the shape and bound of
tests/test_gpu_parity.py::test_witness_second_order."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import smmd_oracle as O  # noqa: E402
from oracle import torch_kernels as T  # noqa: E402


def _inputs(seed=4, b=12, nr=10, nf=9, d=2):
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((b, d))
    R = rng.standard_normal((nr, d))
    F = rng.standard_normal((nf, d)) + 0.5
    g = rng.standard_normal((b, d))
    return H, R, F, g


def _near(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max()
    assert err <= tol * max(1.0, np.abs(ref).max()), '%s: max err %.3e' % (what, err)


@pytest.mark.parametrize('name', O.KERNEL_NAMES)
@pytest.mark.parametrize('d', [1, 2, 5, 16])
def test_kernel_xy_matches_oracle(name, d):
    spec = O.kernel_spec(name)
    A, B, _, _ = _inputs(seed=7, b=19, nr=70, d=d)
    K = T.kernel_xy(spec, torch.tensor(A), torch.tensor(B))
    assert K.dtype == torch.float64
    _near(K.numpy(), O.kernel_matrices(spec, A, B, K_XY_only=True), 1e-12, 'K')


@pytest.mark.parametrize('name', ['rbf', 'mix_rbf', 'mix_rq'])
def test_raw32_matches_gram32(name):
    """Where the kernel reads the Gram pieces through raw alone, raw32 is the
    oracle's gram32 (the same fp32 operation order)."""
    spec = O.kernel_spec(name)
    A, B, _, _ = _inputs(seed=8, b=19, nr=70, d=3)
    A, B = A.astype(np.float32), B.astype(np.float32)
    K =T.kernel_xy(spec, torch.tensor(A), torch.tensor(B), raw32=True).numpy()
    ref = O.kernel_matrices(spec, A, B, K_XY_only=True, gram32=True)
    # np.matmul and torch.matmul may order a 3-term fp32 sum differently: one ulp of raw
    _near(K, ref, 1e-6, 'K raw32')
    plain = T.kernel_xy(spec, torch.tensor(A), torch.tensor(B)).numpy()
    assert np.abs(K - plain).max() > 0          # the fp32 rounding is really in there


@pytest.mark.parametrize('name', O.KERNEL_NAMES)
def test_first_order_matches_oracle(name):
    spec = O.kernel_spec(name)
    H, R, F, g = _inputs()
    # one block: d sum(G * K(A, B)) / d(A, B) against _block_grads
    rng = np.random.default_rng(5)
    G = rng.standard_normal((H.shape[0], R.shape[0]))
    At = torch.tensor(H, requires_grad=True)
    Bt = torch.tensor(R, requires_grad=True)
    (T.kernel_xy(spec, At, Bt) * torch.tensor(G)).sum().backward()
    A1, B1 = (np.tanh(H), np.tanh(R)) if spec.tanh else (H, R)
    AB, sa, sb = O._gram(A1, B1, False)
    rdA, rdB = O._block_grads(spec, A1, B1, AB, sa, sb, G)
    if spec.tanh:
        rdA, rdB = rdA * (1 - A1 ** 2), rdB * (1 - B1 ** 2)
    _near(At.grad.numpy(), rdA, 1e-10, 'gA')
    _near(Bt.grad.numpy(), rdB, 1e-10, 'gB')
    # the witness gradient
    Ht = torch.tensor(H, requires_grad=True)
    dH = T.witness_grad_H(spec, Ht, torch.tensor(R), torch.tensor(F))
    _near(dH.numpy(), O.witness_grad_H(spec, H, R, F), 1e-10, 'dH')
    _near(T.witness(spec, Ht, torch.tensor(R), torch.tensor(F)).detach().numpy(),
          O.witness(spec, H, R, F), 1e-12, 'w')


@pytest.mark.parametrize('name', O.KERNEL_NAMES)
def test_second_order_matches_central_differences(name):
    spec = O.kernel_spec(name)
    H, R, F, g = _inputs()
    ts = [torch.tensor(a, requires_grad=True) for a in (H, R, F)]
    dH = T.witness_grad_H(spec, *ts, create_graph=True)
    (dH * torch.tensor(g)).sum().backward()

    def f(Hh, Rr, Ff):
        return np.sum(O.witness_grad_H(spec, Hh, Rr, Ff) * g)

    args = [H, R, F]
    for idx, arr in enumerate(args):
        num = np.zeros_like(arr)
        for k in np.ndindex(arr.shape):
            e = 1e-5
            ap, am = arr.copy(), arr.copy()
            ap[k] += e
            am[k] -= e
            args_p, args_m = list(args), list(args)
            args_p[idx], args_m[idx] = ap, am
            num[k] = (f(*args_p) - f(*args_m)) / (2 * e)
        # dot: dH does not depend on H, autograd leaves that gradient unset
        got = np.zeros_like(arr) if ts[idx].grad is None else ts[idx].grad.numpy()
        err = np.abs(got - num)
        lim = 2e-3 * max(np.abs(num).max(), 1e-6) + 2e-3 * np.abs(num)
        assert (err <= lim).all(), 'arg %d: max err %.3e' % (idx, err.max())
