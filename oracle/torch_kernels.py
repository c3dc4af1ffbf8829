"""The kernel family in plain torch float64 -- TEST INFRASTRUCTURE ONLY.

``kernel_xy`` restates ``smmd_oracle.kernel_matrices(..., K_XY_only=True)``
formula for formula (gan/core/mmd.py:12, :18-188): the Gram expansion
``-2ab + |a|^2 + |b|^2``, the clamp at 0, ``mysqrt``'s ``+1e-5``, ``tanh`` of
the inputs and ``add_dot``.  ``torch.autograd`` then gives the first and the
second order of anything built from it, with no finite differences; the clamp
is ``torch.clamp(min=0)``, whose backward passes the gradient on ties as
``tf.maximum`` does for its first argument.

``raw32=True`` also forms the Gram pieces in float32 on the CPU, in the
operation order of mmd.py:67, and adds the difference to the float64 ``raw``
as a detached constant: values then see the fp32 cancellation that
``gram32=True`` gives the numpy oracle, while every derivative flows through
the float64 graph.  Comparing the two tells an ill-conditioned input (near
coincident points under the distance kernel's square root) from a wrong
kernel.
"""
from __future__ import annotations

import torch

from .smmd_oracle import EPS, KernelSpec


def _f64(t):
    if torch.is_tensor(t):
        return t if t.dtype == torch.float64 else t.double()
    return torch.as_tensor(t, dtype=torch.float64)


def _mysqrt(x):
    """sqrt(max(x + eps, 0))  (gan/core/mmd.py:12)."""
    return torch.sqrt(torch.clamp(x + EPS, min=0.0))


def kernel_xy(spec: KernelSpec, A, B, raw32=False):
    """K(A, B) [na, nb] in float64, differentiable in A and B."""
    A, B = _f64(A), _f64(B)
    if spec.tanh:
        A, B = torch.tanh(A), torch.tanh(B)
    AB = A @ B.t()
    sa = (A * A).sum(1)
    sb = (B * B).sum(1)
    raw = -2.0 * AB + sa[:, None] + sb[None, :]           # mmd.py:67 (pre-clamp)
    if raw32:
        A32, B32 = A.detach().float(), B.detach().float()
        r32 = (-2.0 * (A32 @ B32.t()) + (A32 * A32).sum(1)[:, None]) + (B32 * B32).sum(1)[None, :]
        raw = raw + (r32.double() - raw.detach())
    if spec.kind == 'rbf':
        R = torch.clamp(raw, min=0.0)
        K = torch.zeros_like(R)
        for sigma, wt in zip(spec.params, spec.wts):
            K = K + wt * torch.exp(-(1.0 / (2.0 * sigma ** 2)) * R)       # mmd.py:69-70
        return K
    if spec.kind == 'rq':
        R = torch.clamp(raw, min=0.0)
        K = torch.zeros_like(R)
        for alpha, wt in zip(spec.params, spec.wts):
            K = K + wt * torch.exp(-alpha * torch.log(1.0 + R / (2.0 * alpha)))   # mmd.py:166-167
        if spec.add_dot > 0:                                              # mmd.py:168-169
            K = K + spec.add_dot * AB
        return K
    if spec.kind == 'distance':                                           # mmd.py:29
        return _mysqrt(sa)[:, None] + _mysqrt(sb)[None, :] - _mysqrt(raw)
    if spec.kind == 'dot':                                                # mmd.py:45
        return AB
    raise ValueError(spec.kind)


def witness(spec: KernelSpec, H, R, F, raw32=False):
    """witness_i = mean_j K(h_i, r_j) - mean_j K(h_i, f_j)  (model.py:336-338)."""
    return kernel_xy(spec, H, R, raw32).mean(1) - kernel_xy(spec, H, F, raw32).mean(1)


def witness_grad_H(spec: KernelSpec, H, R, F, create_graph=False, raw32=False):
    """d sum_i witness_i / d H by autograd (H must require grad); with
    ``create_graph`` the result is differentiable in H, R and F."""
    dH, = torch.autograd.grad(witness(spec, H, R, F, raw32).sum(), H, create_graph=create_graph)
    return dH
