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
* ``cramer_head_loss`` / ``cramer_seed``: the loss side of the Cramer GAN
  (gan/core/cramer.py:81-96): the energy-distance head with its row gradients
  in one launch, the penalty's seed and the seed's backward in one each.
* ``sobolev_head_loss`` / ``weight_decay``: the loss side of the Sobolev GAN
  (gan/core/sobolevgan_gp.py:16-42): the constraint head and the decay over the
  flat parameter buffer, one launch forward and one backward each.
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


# ---------------------------------------------------------------------------
# the loss side of the Cramer GAN (csrc/smmd_cramer.hip): the energy-distance
# head with the row gradients of both losses in one launch, and the penalty's
# seed with its own backward.  SMMD_CRAMER_FUSED=0 routes them through plain
# tensor ops written with safer_norm (A/B); CPU or non-fp32 tensors take that
# path too, so the model also builds and steps without a GPU.
# ---------------------------------------------------------------------------
CRAMER_FUSED = os.environ.get('SMMD_CRAMER_FUSED', '1') != '0'
CRAMER_VARIANTS = {'cramer': 0, 'reddit_cramer': 1}


def _cramer_fused(*tensors):
    return CRAMER_FUSED and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _same_rows(what, *tensors):
    if any(t.dim() != 2 or t.shape != tensors[0].shape for t in tensors):
        raise ValueError('%s: the batches are subtracted row by row and need one [b, d] shape '
                         '(got %s)' % (what, ', '.join(str(tuple(t.shape)) for t in tensors)))


class _CramerHead(torch.autograd.Function):
    """(d_base, g_loss) of the Cramer head and, from the same launch, the row
    gradients of the losses in ``want`` (bit 0 d_base, bit 1 g_loss); the
    backward scales them by the upstream scalars."""

    @staticmethod
    def forward(ctx, G, G2, X, variant, eps, want):
        dev = G.device
        g, g2, x = (t.detach().contiguous() for t in (G, G2, X))
        b, d = g.shape
        L = _lib.lib()
        out = torch.empty(2, device=dev, dtype=torch.float32)
        sets = [[torch.empty_like(g) for _ in range(3)] if want & bit else [None] * 3
                for bit in (1, 2)]
        ws = _lib.workspace('cramer_head', L.smmd_cramer_head_workspace_bytes(b, d), dev)
        _lib.add_bytes('smmd_cramer_head_fwd', (3 + 3 * bin(want).count('1')) * g.numel() * 4)
        with _lib.timed('smmd_cramer_head_fwd'):
            st = L.smmd_cramer_head_fwd(_lib.ptr(g), _lib.ptr(g2), _lib.ptr(x), b, d, variant,
                                        float(eps), want, _lib.ptr(out),
                                        *[_lib.ptr(t) for t in sets[0] + sets[1]],
                                        _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
        _lib.check(st, 'smmd_cramer_head_fwd')
        ctx.save_for_backward(*[t for t in sets[0] + sets[1] if t is not None])
        ctx.want = want
        ctx.set_materialize_grads(False)
        d_base, g_loss = out.unbind(0)
        return d_base, g_loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go_d, go_g):
        saved = list(ctx.saved_tensors)
        grads = [None, None, None]
        for bit, go, name in ((1, go_d, 'd_base'), (2, go_g, 'g_loss')):
            if not ctx.want & bit:
                if go is not None:
                    raise RuntimeError('cramer_head_loss: %s is differentiated but its '
                                       'gradients were not requested (want=%d)' % (name, ctx.want))
                continue
            rows, saved = saved[:3], saved[3:]
            if go is None:
                continue
            for k in range(3):
                if ctx.needs_input_grad[k]:
                    t = go * rows[k]
                    grads[k] = t if grads[k] is None else grads[k] + t
        return (*grads, None, None, None)


def cramer_head_loss(G, G2, images, variant, eps=_eps, want=None):
    """The Cramer GAN's losses on critic outputs [b, d] of a generated batch,
    a second generated batch and the real batch, n = safer_norm over a row:
    'cramer' (cramer.py:85-88): g_loss = mean(-n(G - G2) + n(G - X) + n(G2 - X)),
    d_base = mean(-n(X - G) + n(X) + n(G2 - G) - n(G2)); 'reddit_cramer'
    (cramer.py:90-92): g_loss = mean((n(X - G) - n(X)) - (n(G - G2) - n(G))),
    d_base = -g_loss.  Returns (d_base, g_loss), 0-dim, differentiable once in
    all three inputs.  ``want``: the losses that will be differentiated (bit 0
    d_base, bit 1 g_loss; default both when an input requires grad): the
    kernel writes only those row gradients, and differentiating the other
    loss raises."""
    v = CRAMER_VARIANTS.get(variant, variant)
    if v not in (0, 1):
        raise ValueError("variant must be 'cramer' or 'reddit_cramer'")
    _same_rows('cramer_head_loss', G, G2, images)
    if not _cramer_fused(G, G2, images):
        def n(t):
            return safer_norm(t, axis=1, epsilon=eps)
        if v == 0:
            g_loss = torch.mean(-n(G - G2) + n(G - images) + n(G2 - images))
            d_base = torch.mean(-n(images - G) + n(images) + n(G2 - G) - n(G2))
            return d_base, g_loss
        g_loss = torch.mean((n(images - G) - n(images)) - (n(G - G2) - n(G)))
        return -g_loss, g_loss
    if want is None:
        want = 3 if any(t.requires_grad for t in (G, G2, images)) else 1
    if want not in (1, 2, 3):
        raise ValueError('want must be 1, 2 or 3')
    return _CramerHead.apply(G, G2, images, v, float(eps), want)


class _CramerSeed(torch.autograd.Function):
    """U = (H - G) / n(H - G) - H / n(H) per row; the backward (one launch)
    sends an upstream W through the two normalisations."""

    @staticmethod
    def forward(ctx, H, G, eps):
        dev = H.device
        h, g = H.detach().contiguous(), G.detach().contiguous()
        bs, d = h.shape
        U = torch.empty_like(h)
        norms = torch.empty(bs, 2, device=dev, dtype=torch.float64)
        with _lib.timed('smmd_cramer_seed_fwd'):
            st = _lib.lib().smmd_cramer_seed_fwd(_lib.ptr(h), _lib.ptr(g), bs, d, float(eps),
                                                 _lib.ptr(U), _lib.ptr(norms),
                                                 _lib.stream_handle(dev))
        _lib.check(st, 'smmd_cramer_seed_fwd')
        ctx.save_for_backward(h, g, norms)
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, W):
        h, g, norms = ctx.saved_tensors
        bs, d = h.shape
        w = W.contiguous().to(torch.float32)
        gH, gG = torch.empty_like(h), torch.empty_like(h)
        with _lib.timed('smmd_cramer_seed_bwd'):
            st = _lib.lib().smmd_cramer_seed_bwd(_lib.ptr(h), _lib.ptr(g), _lib.ptr(norms),
                                                 _lib.ptr(w), bs, d, _lib.ptr(gH), _lib.ptr(gG),
                                                 _lib.stream_handle(h.device))
        _lib.check(st, 'smmd_cramer_seed_bwd')
        return gH, gG, None


def cramer_seed(H, G, eps=_eps):
    """The seed of the Cramer penalty, U [bs, d] = d sum_i(n(H_i - G_i) -
    n(H_i)) / dH for critic outputs H of the interpolates and G of the
    generated batch's first bs rows (cramer.py:81, :88, :96: the grad_outputs
    of tf.gradients(to_penalize, x_hat_data)).  It depends on the critic, so
    it is differentiable once in H and G (the penalty's gradient reaches the
    critic through it)."""
    _same_rows('cramer_seed', H, G)
    if not _cramer_fused(H, G):
        a = H - G
        return (a / safer_norm(a, axis=1, keep_dims=True, epsilon=eps)
                - H / safer_norm(H, axis=1, keep_dims=True, epsilon=eps))
    return _CramerSeed.apply(H, G, float(eps))


# ---------------------------------------------------------------------------
# the loss side of the Sobolev GAN (csrc/smmd_sobolev.hip): the critic update's
# whole head (both energies, the constraint, the augmented-Lagrangian term, the
# next multiplier) in one launch forward and one backward, and the weight decay
# over the optimizer's flat parameter buffer in one launch each way.
# SMMD_SOBOLEV_FUSED=0 routes both through plain tensor ops (A/B); CPU or
# non-fp32 tensors take that path too, so the model also builds without a GPU.
# ---------------------------------------------------------------------------
SOBOLEV_FUSED = os.environ.get('SMMD_SOBOLEV_FUSED', '1') != '0'


def _sobolev_fused(*tensors):
    return SOBOLEV_FUSED and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _dense(t):
    """t when it is dense in either memory format, else a contiguous copy."""
    return t if t.is_contiguous() or _is_channels_last(t) else t.contiguous()


class _SobolevHead(torch.autograd.Function):
    """(d_base, g_loss, c, mult) in one launch; the backward (one launch)
    reads mult from the saved outputs on the device."""

    @staticmethod
    def forward(ctx, d_real, d_fake, g_real, g_fake, lam, rho):
        dev = g_real.device
        xr = d_real.detach().reshape(-1).contiguous()
        xf = d_fake.detach().reshape(-1).contiguous()
        gr, gf = _dense(g_real.detach()), _dense(g_fake.detach())
        b_real, b_fake = gr.shape[0], gf.shape[0]
        per = gr.numel() // b_real
        L = _lib.lib()
        out = torch.empty(6, device=dev, dtype=torch.float32)
        ws = _lib.workspace('sobolev_head', L.smmd_sobolev_workspace_bytes(b_real, b_fake, per),
                            dev)
        _lib.add_bytes('smmd_sobolev_fwd', (gr.numel() + gf.numel()) * 4)
        with _lib.timed('smmd_sobolev_fwd'):
            st = L.smmd_sobolev_fwd(_lib.ptr(gr), _lib.ptr(gf), _lib.ptr(xr), _lib.ptr(xf), b_real,
                                    b_fake, per, _lib.ptr(lam), float(rho), _lib.ptr(out),
                                    _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
        _lib.check(st, 'smmd_sobolev_fwd')
        ctx.save_for_backward(gr, gf, out)
        ctx.cfg = (b_real, b_fake, per, d_real.shape, d_fake.shape)
        d_base, g_loss, c, mult = out[:4].unbind(0)
        ctx.mark_non_differentiable(g_loss, c, mult)
        return d_base, g_loss, c, mult

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go, *unused):
        gr, gf, out = ctx.saved_tensors
        b_real, b_fake, per, sr, sf = ctx.cfg
        dev = gr.device
        go = go.reshape(1).contiguous().to(torch.float32)
        dgr, dgf = torch.empty_like(gr), torch.empty_like(gf)      # the inputs' strides (dense)
        ddr = torch.empty(b_real, device=dev, dtype=torch.float32)
        ddf = torch.empty(b_fake, device=dev, dtype=torch.float32)
        _lib.add_bytes('smmd_sobolev_bwd', 2 * (gr.numel() + gf.numel()) * 4)
        with _lib.timed('smmd_sobolev_bwd'):
            st = _lib.lib().smmd_sobolev_bwd(_lib.ptr(gr), _lib.ptr(gf), b_real, b_fake, per,
                                             _lib.ptr(out), _lib.ptr(go), _lib.ptr(dgr),
                                             _lib.ptr(dgf), _lib.ptr(ddr), _lib.ptr(ddf),
                                             _lib.stream_handle(dev))
        _lib.check(st, 'smmd_sobolev_bwd')
        return ddr.view(sr), ddf.view(sf), dgr, dgf, None, None


def sobolev_head_loss(d_real, d_fake, g_real, g_fake, lam, rho):
    """The Sobolev GAN critic loss before the weight decay, on the critic
    outputs d_real [b_r, 1], d_fake [b_f, 1] and the critic's input gradients
    g_real = d sum(D(real)) / d real, g_fake = d sum(D(fake)) / d fake (dense,
    either memory format): with e_r = sum(g_real^2) / b_r, e_f = sum(g_fake^2)
    / b_f (sobolevgan_gp.py:19-20) and c = e_r / 2 + e_f / 2 - 1 (:22),

        d_base = mean(d_fake) - mean(d_real) + lam c + rho c^2 / 2   (:29, :40)
        g_loss = -mean(d_fake)                                        (:30)
        mult   = lam + rho c                                          (:42)

    ``lam``: a one-element tensor (on the device: read there), ``rho`` a host
    float.  Returns (d_base, g_loss, c, mult), all 0-dim; d_base is
    differentiable once in the four tensors (the rest of a critic update's
    chain is the critic's own second-order rule), the other three are values:
    mult is both d d_base / d c and the next multiplier."""
    b_real, b_fake = g_real.shape[0], g_fake.shape[0]
    if (d_real.numel() != b_real or d_fake.numel() != b_fake
            or g_real.numel() // b_real != g_fake.numel() // b_fake or lam.numel() != 1):
        raise ValueError('sobolev_head_loss: d_real %s, d_fake %s, g_real %s, g_fake %s, lam %s'
                         % tuple(tuple(t.shape) for t in (d_real, d_fake, g_real, g_fake, lam)))
    if not _sobolev_fused(d_real, d_fake, g_real, g_fake, lam):
        lam = lam.detach().reshape(()).to(g_real.dtype)
        e_real = (g_real * g_real).sum() / b_real
        e_fake = (g_fake * g_fake).sum() / b_fake
        c = 0.5 * e_real + 0.5 * e_fake - 1.0
        mf = d_fake.mean()
        d_base = mf - d_real.mean() + lam * c + 0.5 * rho * c * c
        return d_base, (-mf).detach(), c.detach(), (lam + rho * c).detach()
    return _SobolevHead.apply(d_real, d_fake, g_real, g_fake, lam.detach(), float(rho))


def _flat_offset(p, flat):
    """Element offset of parameter p inside the flat buffer it is a view of."""
    o, r = divmod(p.data_ptr() - flat.data_ptr(), flat.element_size())
    if r or o < 0 or o + p.numel() > flat.numel() or p.dtype != flat.dtype:
        raise ValueError('weight_decay: a parameter %s is not a view of the flat buffer'
                         % (tuple(p.shape),))
    return o


class _WeightDecay(torch.autograd.Function):
    """sum_s coef_s sum_{i in s} flat_i^2 in one launch; the backward writes
    one dflat (one launch) and hands every parameter its view of it."""

    @staticmethod
    def forward(ctx, flat, offsets, coefs, *params):
        dev = flat.device
        L = _lib.lib()
        n = flat.numel()
        out = torch.empty(1, device=dev, dtype=torch.float32)
        ws = _lib.workspace('decay', L.smmd_decay_workspace_bytes(n), dev)
        _lib.add_bytes('smmd_decay_fwd', n * 4)
        with _lib.timed('smmd_decay_fwd'):
            st = L.smmd_decay_fwd(_lib.ptr(flat), n, _lib.ptr(offsets), _lib.ptr(coefs),
                                  coefs.numel(), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_handle(dev))
        _lib.check(st, 'smmd_decay_fwd')
        ctx.save_for_backward(flat, offsets, coefs)
        ctx.views = [(p.shape, p.stride(), _flat_offset(p, flat)) for p in params]
        return out.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        flat, offsets, coefs = ctx.saved_tensors
        n = flat.numel()
        go = go.reshape(1).contiguous().to(torch.float32)
        dflat = torch.empty_like(flat)
        _lib.add_bytes('smmd_decay_bwd', 2 * n * 4)
        with _lib.timed('smmd_decay_bwd'):
            st = _lib.lib().smmd_decay_bwd(_lib.ptr(flat), n, _lib.ptr(offsets), _lib.ptr(coefs),
                                           coefs.numel(), _lib.ptr(go), _lib.ptr(dflat),
                                           _lib.stream_handle(flat.device))
        _lib.check(st, 'smmd_decay_bwd')
        return (None, None, None,
                *[torch.as_strided(dflat, sh, st_, o) for sh, st_, o in ctx.views])


def weight_decay(params, flat, offsets, coefs):
    """sum over segments s of coefs[s] * sum(flat[offsets[s]:offsets[s + 1]]^2)
    (sobolevgan_gp.py:32-37, :41) for ``params`` that are views of the 1-D
    buffer ``flat`` (FlatAdam's ``flat_param``): ``offsets`` [nseg + 1] int64
    ascending element offsets and ``coefs`` [nseg] of flat's dtype, both on
    flat's device; every parameter lies inside one segment.  A 0-dim tensor,
    differentiable once with respect to each parameter: 2 coef_s p."""
    params = list(params)
    if (flat.dim() != 1 or not flat.is_contiguous() or offsets.dtype != torch.int64
            or offsets.numel() != coefs.numel() + 1 or coefs.numel() < 1):
        raise ValueError('weight_decay: flat %s, offsets %s %s, coefs %s'
                         % (tuple(flat.shape), tuple(offsets.shape), offsets.dtype,
                            tuple(coefs.shape)))
    if _sobolev_fused(flat, coefs) and offsets.is_cuda:
        return _WeightDecay.apply(flat, offsets.contiguous(), coefs.contiguous(), *params)
    import bisect
    host = getattr(offsets, '_smmd_host', None)        # (read back once per table)
    if host is None:
        host = offsets._smmd_host = (offsets.tolist(), coefs.tolist())
    offs, cfs = host
    total = flat.new_zeros(())
    for p in params:
        o = _flat_offset(p, flat)
        s = bisect.bisect_right(offs, o) - 1
        if not (0 <= s < len(cfs) and o + p.numel() <= offs[s + 1]):
            raise ValueError('weight_decay: a parameter %s at offset %d lies in no one segment'
                             % (tuple(p.shape), o))
        total = total + cfs[s] * (p * p).sum()
    return total
