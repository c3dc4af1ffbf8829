"""The original GAN loss (gan/core/gan.py) on the HIP critic head.

``-model gan -with_sn true`` is SN-GAN, the baseline the Scaled-MMD paper
compares against.  The loss is one launch (ops.critic_head_loss, csrc
smmd_critic_head_fwd): the softplus means and their row gradients together.
"""
from __future__ import annotations

from . import ops
from .model import MMD_GAN


class HeadModel(MMD_GAN):
    """What the critic-head models (GAN, WGAN_GP) share: dof_dim forced to 1
    (gan.py:6, wgan_gp.py:6), no scaling regulariser, and the limits of this
    build -- tower-mode data parallel only, no step graphs."""

    def __init__(self, config, device=None, process_group=None, dp_mode='tower', **kw):
        if dp_mode == 'global':
            raise NotImplementedError(
                "%s: dp_mode='global' is not built for this model (its loss is a mean over the "
                "local batch; use dp_mode='tower')" % type(self).__name__)
        config.dof_dim = 1
        super().__init__(config, device=device, process_group=process_group, dp_mode=dp_mode,
                         **kw)

    def _scaling_ahead(self):
        return False                 # neither reference class calls add_scaling

    def enable_graphs(self, on=True):
        if on:
            raise NotImplementedError(
                '%s: step graphs are not built for this model (the penalty\'s critic call and '
                'its alpha draw are unproven under capture)' % type(self).__name__)
        super().enable_graphs(False)


class GAN(HeadModel):
    """gan.py:5-12: d_loss = mean(softplus(-D(images)) + softplus(D(G))),
    g_loss = mean(softplus(-D(G)))."""

    def __init__(self, config, **kw):
        super().__init__(config, **kw)
        self.optim_name = 'gan%d_loss' % int(config.gradient_penalty)

    def set_loss(self, G, images):
        self.d_loss, self.g_loss = ops.critic_head_loss(images, G, 1)      # gan.py:10-11
        self.optim_name = 'gan%d_loss' % int(self.config.gradient_penalty)


__all__ = ['GAN', 'HeadModel']
