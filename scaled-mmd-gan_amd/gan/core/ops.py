"""Hot-path helpers of gan/core/ops.py and the scaled-loss op.

* ``safer_norm`` / ``sq_sum`` / ``dot``: small reductions (gan/core/ops.py:
  203-225) used by the gradient penalty; plain tensor reductions.
* ``jacobian_columns`` + ``scaled_loss``: ``squared_norm_jacobian``
  (ops.py:228-233) fused with ``add_scaling`` (gan/core/model.py:366-403) and
  ``apply_scaling`` (gan/core/smmd.py:21-23, :40-42) in libsmmd_hip: one
  HBM pass over the input-gradient, one single-block finalize, and a one-pass
  backward that feeds PyTorch's double-backward through the critic.
* ``gp_interpolate`` / ``slope_penalty`` / ``critic_head_loss``: the loss side
  of the GAN and WGAN-GP baselines (gan/core/gan.py:10-11,
  gan/core/wgan_gp.py:10-25), one HIP launch forward and one backward each.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist

from . import _lib
from .collectives import all_reduce_
from .convops import input_grad_only
from .mmd import _eps


def safer_norm(tensor, axis=None, keep_dims=False, epsilon=_eps):
    """sqrt(sum(t^2, axis) + eps)  (gan/core/ops.py:203-206)."""
    sq = tensor * tensor
    if axis is None:
        s = sq.sum()
    else:
        s = sq.sum(dim=axis, keepdim=keep_dims)
    return torch.sqrt(s + epsilon)


def sq_sum(t, name=None):
    """sum(t ** 2)  (gan/core/ops.py:209-213)."""
    return (t * t).sum()


def dot(x, y, name=None):
    """<x, y> of two vectors  (gan/core/ops.py:216-225)."""
    if x.dim() != 1 or y.dim() != 1:
        raise ValueError('dot expects rank-1 tensors')
    return (x * y).sum()


_SEEDS = {}


def grad_seed(y, i=None):
    """The gradient d(sum y[:, i]) / dy (i None: d(sum y) / dy) as a constant
    tensor, kept per shape outside a graph capture: seeding autograd with it
    gives the same gradient as differentiating the select and the sum -- the
    same ones in the same places -- without their zero, copy and fill
    kernels.  (Autograd never adds into a seed it does not own alone.)"""
    key = (tuple(y.shape), y.dtype, y.device, i)
    t = _SEEDS.get(key)
    if t is None:
        if i is None:
            t = torch.ones(y.shape, dtype=y.dtype, device=y.device)
        else:
            t = torch.zeros(y.shape, dtype=y.dtype, device=y.device)
            t[:, i] = 1
        if y.is_cuda and torch.cuda.is_current_stream_capturing():
            return t
        _SEEDS[key] = t
    return t


def jacobian_columns(y, x, create_graph=True):
    """Stack of d(sum_b y[b, i]) / dx for every critic output column i
    (gan/core/ops.py:230-231): returns [d, *x.shape].  The critic has no
    cross-sample coupling in the configs (no BN in D), so
    row b of column i is d y[b, i] / d x[b].  Each column's pass is seeded
    with grad_seed(y, i), the gradient of y[:, i].sum() w.r.t. y."""
    d = y.shape[1]
    cols = []
    for i in range(d):
        with input_grad_only():       # no weight-gradient kernels in this pass
            g, = torch.autograd.grad(y, x, grad_outputs=grad_seed(y, i),
                                     create_graph=create_graph, retain_graph=True)
        cols.append(g)
    return torch.stack(cols, 0) if d > 1 else cols[0].unsqueeze(0)


class _ScaledLoss(torch.autograd.Function):
    """g_loss = base * f(scale), scale = 1 / (sc * Q + 1),
    Q = mean_b sum_c ||jac[c, b]||^2 (+ mean(feat^2) for 'value_and_grad'),
    f = id (SMMD) or sqrt (SWGAN)."""

    @staticmethod
    def forward(ctx, base, jac, feat, sc, variant, sqrt_scale, b_total, group, pre):
        _lib.require_cuda(base, jac, feat)
        jac = jac.contiguous()
        n_cols, b = jac.shape[0], jac.shape[1]
        per = jac[0, 0].numel()
        dev = jac.device
        L = _lib.lib()
        base = base.reshape(1).contiguous()
        feat_c = feat.contiguous() if feat is not None else None
        dof = feat_c.shape[1] if feat_c is not None else 0
        s = _lib.stream_handle(dev)
        per_sample = torch.empty(b, device=dev, dtype=torch.float32)
        if pre is not None:
            # global J / nD already known (gathered with the step's features):
            # only the single-thread finalize runs
            out = torch.zeros(8, device=dev, dtype=torch.float32)
            out[3:5] = pre
            out[5:6] = base.detach()
            _lib.check(L.smmd_scaled_loss_finalize(_lib.ptr(out), float(sc), variant,
                                                   sqrt_scale, s), 'smmd_scaled_loss_finalize')
            group = None
        else:
            out = torch.empty(8, device=dev, dtype=torch.float32)
            nbytes = L.smmd_scaled_loss_workspace_bytes(n_cols * b, per)
            ws = _lib.workspace('scaled_loss', nbytes, dev)
            args = (_lib.ptr(jac), n_cols, b, b_total, per, _lib.ptr(feat_c), dof,
                    _lib.ptr(base), float(sc), variant, sqrt_scale, _lib.ptr(out),
                    _lib.ptr(per_sample), _lib.ptr(ws), ws.numel(), s)
            with _lib.timed('smmd_scaled_loss_fwd'):
                st = L.smmd_scaled_loss_fwd(*args)
            _lib.check(st, 'smmd_scaled_loss_fwd')
        if group is not None:
            # J and nD are partial means over the global batch: sum them
            all_reduce_(out[3:5], group)
            _lib.check(L.smmd_scaled_loss_finalize(_lib.ptr(out), float(sc), variant,
                                                   sqrt_scale, s), 'smmd_scaled_loss_finalize')
        ctx.save_for_backward(jac, feat_c, out)
        ctx.cfg = (n_cols, b, b_total, per, dof, float(sc), variant, sqrt_scale)
        ctx.mark_non_differentiable(out, per_sample)
        return out[0].view(()), out, per_sample

    @staticmethod
    def backward(ctx, g_gloss, g_out, g_ps):
        jac, feat, out = ctx.saved_tensors
        n_cols, b, b_total, per, dof, sc, variant, sqrt_scale = ctx.cfg
        dev = jac.device
        go = g_gloss.reshape(1).contiguous().to(torch.float32)
        d_base = torch.empty(1, device=dev, dtype=torch.float32)
        gjac = torch.empty_like(jac)
        gfeat = torch.empty_like(feat) if (feat is not None and variant == 1) else None
        args = (_lib.ptr(jac), n_cols, b, b_total, per, _lib.ptr(feat), dof, _lib.ptr(out), sc,
                variant, sqrt_scale, _lib.ptr(go), _lib.ptr(d_base), _lib.ptr(gjac),
                _lib.ptr(gfeat), _lib.stream_handle(dev))
        with _lib.timed('smmd_scaled_loss_bwd'):
            st = _lib.lib().smmd_scaled_loss_bwd(*args)
        _lib.check(st, 'smmd_scaled_loss_bwd')
        if feat is not None and gfeat is None:
            gfeat = torch.zeros_like(feat)
        return d_base.view(()), gjac, gfeat, None, None, None, None, None, None


def _b_total(jac, process_group):
    from .collectives import is_dp
    group = process_group if is_dp(process_group) else None
    return group, jac.shape[1] * (dist.get_world_size(group) if group is not None else 1)


def scaling_partials(jac, feat=None, variant='grad', process_group=None):
    """This rank's share of (J, nD) over the global batch -- sum over its rows
    divided by the global batch size -- as a detached [2] tensor: the partials
    a collectives.StepExchange gathers with the critic features so the scale
    needs no all-reduce of its own (``scaled_loss(..., pre=sum of them)``)."""
    v = {'grad': 0, 'value_and_grad': 1}[variant]
    _, b_total = _b_total(jac, process_group)
    jac = jac.detach().contiguous()
    n_cols, b, per = jac.shape[0], jac.shape[1], jac[0, 0].numel()
    feat_c = feat.detach().contiguous() if (feat is not None and v == 1) else None
    dof = feat_c.shape[1] if feat_c is not None else 0
    dev = jac.device
    L = _lib.lib()
    out = torch.empty(8, device=dev, dtype=torch.float32)
    ws = _lib.workspace('scaled_loss', L.smmd_scaled_loss_workspace_bytes(n_cols * b, per), dev)
    with _lib.timed('smmd_scaled_loss_fwd'):
        st = L.smmd_scaled_loss_fwd(_lib.ptr(jac), n_cols, b, b_total, per, _lib.ptr(feat_c), dof,
                                    None, 0.0, v, 0, _lib.ptr(out), None, _lib.ptr(ws),
                                    ws.numel(), _lib.stream_handle(dev))
    _lib.check(st, 'smmd_scaled_loss_fwd')
    return out[3:5]


def scaled_loss(base, jac, feat=None, sc=10.0, variant='grad', sqrt_scale=False,
                process_group=None, pre=None):
    """Apply the scaling regulariser to ``base`` (mmd2 for SMMD, the critic
    mean difference for SWGAN).  ``jac`` = jacobian_columns(d_images, images).

    Returns (g_loss, aux) with aux a detached 8-vector
    [g_loss, d_loss, scale, J, norm_discriminator, base, 0, 0] and, in the
    all-gather mode, J / nD over the global batch: all-reduced here, or
    ``pre`` = their global values already gathered (collectives.StepExchange)."""
    v = {'grad': 0, 'value_and_grad': 1}[variant]
    if v == 1 and feat is None:
        raise ValueError("scaling_variant 'value_and_grad' needs the critic output")
    group, b_total = _b_total(jac, process_group)
    g, out, _ = _ScaledLoss.apply(base, jac, feat if v == 1 else None, sc, v,
                                  1 if sqrt_scale else 0, b_total, group, pre)
    return g, out


class _ScaleFactor(torch.autograd.Function):
    """scale = 1 / (sc * Q + 1) alone (model.py:387-390), for an overridden
    apply_scaling: the same HIP pass as _ScaledLoss without a base loss.  The
    backward reuses smmd_scaled_loss_bwd with base := 1 and f = id, whose
    dL/dQ = go * base * (-sc scale^2) is then exactly d scale / dQ * go."""

    @staticmethod
    def forward(ctx, jac, feat, sc, variant, b_total, group, pre):
        _lib.require_cuda(jac, feat)
        jac = jac.contiguous()
        n_cols, b = jac.shape[0], jac.shape[1]
        per = jac[0, 0].numel()
        dev = jac.device
        L = _lib.lib()
        feat_c = feat.contiguous() if feat is not None else None
        dof = feat_c.shape[1] if feat_c is not None else 0
        s = _lib.stream_handle(dev)
        if pre is not None:
            out = torch.zeros(8, device=dev, dtype=torch.float32)
            out[3:5] = pre
            _lib.check(L.smmd_scaled_loss_finalize(_lib.ptr(out), float(sc), variant, 0, s),
                       'smmd_scaled_loss_finalize')
            group = None
        else:
            out = torch.empty(8, device=dev, dtype=torch.float32)
            per_sample = torch.empty(b, device=dev, dtype=torch.float32)
            ws = _lib.workspace('scaled_loss',
                                L.smmd_scaled_loss_workspace_bytes(n_cols * b, per), dev)
            with _lib.timed('smmd_scaled_loss_fwd'):
                st = L.smmd_scaled_loss_fwd(_lib.ptr(jac), n_cols, b, b_total, per,
                                            _lib.ptr(feat_c), dof, None, float(sc), variant, 0,
                                            _lib.ptr(out), _lib.ptr(per_sample), _lib.ptr(ws),
                                            ws.numel(), s)
            _lib.check(st, 'smmd_scaled_loss_fwd')
        if group is not None:
            all_reduce_(out[3:5], group)
            _lib.check(L.smmd_scaled_loss_finalize(_lib.ptr(out), float(sc), variant, 0, s),
                       'smmd_scaled_loss_finalize')
        ctx.save_for_backward(jac, feat_c, out)
        ctx.cfg = (n_cols, b, b_total, per, dof, float(sc), variant)
        ctx.mark_non_differentiable(out)
        return out[2].clone().view(()), out

    @staticmethod
    def backward(ctx, g_scale, g_out):
        jac, feat, out = ctx.saved_tensors
        n_cols, b, b_total, per, dof, sc, variant = ctx.cfg
        unit = out.clone()
        unit[5] = 1.0                      # base := 1, so dL/dQ = g_scale d scale / dQ
        go = g_scale.reshape(1).contiguous().to(torch.float32)
        gjac = torch.empty_like(jac)
        gfeat = torch.empty_like(feat) if (feat is not None and variant == 1) else None
        with _lib.timed('smmd_scaled_loss_bwd'):
            st = _lib.lib().smmd_scaled_loss_bwd(
                _lib.ptr(jac), n_cols, b, b_total, per, _lib.ptr(feat), dof, _lib.ptr(unit), sc,
                variant, 0, _lib.ptr(go), None, _lib.ptr(gjac), _lib.ptr(gfeat),
                _lib.stream_handle(jac.device))
        _lib.check(st, 'smmd_scaled_loss_bwd')
        if feat is not None and gfeat is None:
            gfeat = torch.zeros_like(feat)
        return gjac, gfeat, None, None, None, None, None


def scaling_factor(jac, feat=None, sc=10.0, variant='grad', process_group=None, pre=None):
    """scale of MMD_GAN.add_scaling (model.py:382-390) as a differentiable
    0-dim tensor, for an ``apply_scaling(scale)`` override.  Returns (scale,
    aux) with aux as in ``scaled_loss`` (g_loss, d_loss and base unset)."""
    v = {'grad': 0, 'value_and_grad': 1}[variant]
    if v == 1 and feat is None:
        raise ValueError("scaling_variant 'value_and_grad' needs the critic output")
    group, b_total = _b_total(jac, process_group)
    scale, out = _ScaleFactor.apply(jac, feat if v == 1 else None, sc, v, b_total, group, pre)
    return scale, out


class _SqNormJac(torch.autograd.Function):
    @staticmethod
    def forward(ctx, jac):
        _lib.require_cuda(jac)
        jac = jac.contiguous()
        n_cols, b = jac.shape[0], jac.shape[1]
        per = jac[0, 0].numel()
        dev = jac.device
        L = _lib.lib()
        out = torch.empty(8, device=dev, dtype=torch.float32)
        per_sample = torch.empty(b, device=dev, dtype=torch.float32)
        ws = _lib.workspace('scaled_loss', L.smmd_scaled_loss_workspace_bytes(n_cols * b, per),
                            dev)
        _lib.check(L.smmd_scaled_loss_fwd(_lib.ptr(jac), n_cols, b, b, per, None, 0, None, 0.0,
                                          0, 0, _lib.ptr(out), _lib.ptr(per_sample), _lib.ptr(ws),
                                          ws.numel(), _lib.stream_handle(dev)),
                   'smmd_scaled_loss_fwd')
        ctx.save_for_backward(jac)
        return per_sample

    @staticmethod
    def backward(ctx, g):
        jac, = ctx.saved_tensors
        return 2.0 * jac * g.view(1, -1, *([1] * (jac.dim() - 2)))


def squared_norm_jacobian(y, x):
    """sum_i ||d y[:, i] / d x||^2 per sample  (gan/core/ops.py:228-233)."""
    return _SqNormJac.apply(jacobian_columns(y, x))


# ---------------------------------------------------------------------------
# the loss side of the GAN / WGAN-GP baselines (csrc/smmd_gp.hip): one launch
# forward and one backward each.  SMMD_GP_FUSED=0 routes them through plain
# tensor ops in the same arithmetic order (A/B); CPU or non-fp32 tensors take
# that path too, so the models also build without a GPU.
# ---------------------------------------------------------------------------
GP_FUSED = os.environ.get('SMMD_GP_FUSED', '1') != '0'


def _gp_fused(*tensors):
    return GP_FUSED and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _is_channels_last(t):
    return (t.dim() == 4 and not t.is_contiguous()
            and t.is_contiguous(memory_format=torch.channels_last))


def gp_interpolate(real, fake, alpha, form=0):
    """The gradient penalty's interpolates between two batches, alpha one
    number per sample ([b] or [b, 1, 1, 1]): form 0 is real + alpha * (fake -
    real) (wgan_gp.py:13-14), form 1 (1 - alpha) * real + alpha * fake
    (cramer.py:78, model.py:333-334).  Not differentiable (every caller
    detaches both batches); returns a new tensor in ``real``'s memory format,
    ready to be made a leaf."""
    if form not in (0, 1):
        raise ValueError('form must be 0 or 1')
    real, fake, alpha = real.detach(), fake.detach(), alpha.detach()
    b = real.shape[0]
    if fake.shape != real.shape or alpha.numel() != b:
        raise ValueError('gp_interpolate: real %s, fake %s, alpha %s'
                         % (tuple(real.shape), tuple(fake.shape), tuple(alpha.shape)))
    if not _gp_fused(real, fake, alpha):
        a = alpha.reshape([b] + [1] * (real.dim() - 1))
        if form == 0:
            return real + a * (fake - real)
        return (1.0 - a) * real + a * fake
    # dense rows either way: the kernel is told only the row length
    fmt = torch.channels_last if _is_channels_last(real) else torch.contiguous_format
    real = real.contiguous(memory_format=fmt)
    fake = fake.contiguous(memory_format=fmt)
    alpha = alpha.reshape(b).contiguous()
    out = torch.empty_like(real)
    per = real.numel() // b
    _lib.add_bytes('smmd_gp_interp', 3 * real.numel() * 4)
    with _lib.timed('smmd_gp_interp'):
        st = _lib.lib().smmd_gp_interp(_lib.ptr(real), _lib.ptr(fake), _lib.ptr(alpha),
                                       _lib.ptr(out), b, per, form,
                                       _lib.stream_handle(real.device))
    _lib.check(st, 'smmd_gp_interp')
    return out


class _SlopePenalty(torch.autograd.Function):
    """mean over pixels of (sqrt(sum_c g^2 + eps) - 1)^2 for g [b, c, h, w];
    the backward is one elementwise launch from the saved slopes."""

    @staticmethod
    def forward(ctx, g, eps):
        cl = _is_channels_last(g)
        if not cl:
            g = g.contiguous()
        b, c = g.shape[0], g.shape[1]
        hw = g.numel() // (b * c)
        dev = g.device
        L = _lib.lib()
        out = torch.empty(1, device=dev, dtype=torch.float32)
        slopes = torch.empty(b * hw, device=dev, dtype=torch.float32)
        nbytes = L.smmd_gp_slope_workspace_bytes(b, c, hw)
        ws = _lib.workspace('gp_slope', nbytes, dev)
        _lib.add_bytes('smmd_gp_slope_fwd', (g.numel() + slopes.numel()) * 4)
        with _lib.timed('smmd_gp_slope_fwd'):
            st = L.smmd_gp_slope_fwd(_lib.ptr(g), b, c, hw, int(cl), float(eps), _lib.ptr(out),
                                     _lib.ptr(slopes), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_handle(dev))
        _lib.check(st, 'smmd_gp_slope_fwd')
        ctx.save_for_backward(g, slopes)
        ctx.cfg = (b, c, hw, int(cl))
        return out.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        g, slopes = ctx.saved_tensors
        b, c, hw, cl = ctx.cfg
        go = go.reshape(1).contiguous().to(torch.float32)
        dg = torch.empty_like(g)                     # g's strides (dense)
        _lib.add_bytes('smmd_gp_slope_bwd', (2 * g.numel() + slopes.numel()) * 4)
        with _lib.timed('smmd_gp_slope_bwd'):
            st = _lib.lib().smmd_gp_slope_bwd(_lib.ptr(g), _lib.ptr(slopes), b, c, hw, cl,
                                              _lib.ptr(go), _lib.ptr(dg),
                                              _lib.stream_handle(g.device))
        _lib.check(st, 'smmd_gp_slope_bwd')
        return dg, None


def slope_penalty(g, eps=0.0):
    """The gradient penalty of a critic input gradient g [b, c, h, w]:
    mean((slopes - 1)^2), slopes = sqrt(sum over the channel axis of g^2 + eps)
    per pixel (wgan_gp.py:18-19; eps 0 is its plain tf.sqrt, eps 1e-8
    safer_norm).  A 0-dim tensor, differentiable once with respect to g: a
    critic update needs dP/dg only, the rest of the chain being the critic's
    own second-order rule.  The memory format is read from g's strides."""
    if g.dim() < 2:
        raise ValueError('slope_penalty expects [b, c, ...]')
    if not _gp_fused(g):
        s = torch.sqrt((g * g).sum(dim=1) + eps)
        return torch.mean((s - 1.0) ** 2)
    return _SlopePenalty.apply(g, float(eps))


class _CriticHead(torch.autograd.Function):
    """(d_base, g_loss) of the Wasserstein (kind 0) or softplus (kind 1) head
    and, from the same launch, their row gradients; the backward scales them
    by the upstream scalars."""

    @staticmethod
    def forward(ctx, d_real, d_fake, kind):
        dev = d_real.device
        xr = d_real.detach().reshape(-1).contiguous()
        xf = d_fake.detach().reshape(-1).contiguous()
        out = torch.empty(2, device=dev, dtype=torch.float32)
        g_real = torch.empty_like(xr)
        g_fake = torch.empty_like(xf)
        gg_fake = torch.empty_like(xf)
        with _lib.timed('smmd_critic_head_fwd'):
            st = _lib.lib().smmd_critic_head_fwd(_lib.ptr(xr), xr.numel(), _lib.ptr(xf), xf.numel(),
                                                 int(kind), _lib.ptr(out), _lib.ptr(g_real),
                                                 _lib.ptr(g_fake), _lib.ptr(gg_fake),
                                                 _lib.stream_handle(dev))
        _lib.check(st, 'smmd_critic_head_fwd')
        ctx.save_for_backward(g_real, g_fake, gg_fake)
        ctx.shapes = (d_real.shape, d_fake.shape)
        d_base, g_loss = out.unbind(0)
        return d_base, g_loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go_d, go_g):
        g_real, g_fake, gg_fake = ctx.saved_tensors
        sr, sf = ctx.shapes
        return ((go_d * g_real).view(sr), (go_d * g_fake + go_g * gg_fake).view(sf), None)


def critic_head_loss(d_real, d_fake, kind):
    """The critic head on outputs [n, 1]: kind 0, WGAN (wgan_gp.py:24-25):
    d_base = mean(d_fake) - mean(d_real), g_loss = -mean(d_fake); kind 1, GAN
    (gan.py:10-11): d_base = mean(softplus(-d_real)) + mean(softplus(d_fake)),
    g_loss = mean(softplus(-d_fake)).  Returns (d_base, g_loss), both 0-dim
    and differentiable with respect to both critic outputs."""
    if kind not in (0, 1):
        raise ValueError('kind must be 0 (wgan) or 1 (gan)')
    if not _gp_fused(d_real, d_fake):
        if kind == 0:
            mf = d_fake.mean()
            return mf - d_real.mean(), -mf
        sp = torch.nn.functional.softplus
        return sp(-d_real).mean() + sp(d_fake).mean(), sp(-d_fake).mean()
    return _CriticHead.apply(d_real, d_fake, kind)
