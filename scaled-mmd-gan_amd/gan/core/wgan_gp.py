"""WGAN-GP (gan/core/wgan_gp.py) on the HIP loss kernels.

A critic update: the Wasserstein head (one launch), then the penalty --
interpolates (one launch), a third critic call, one input-gradient pass, the
per-pixel slopes and their penalty (one launch forward, one backward).  The
rest of d_loss's gradient, d g / d theta, is the convolutions' own
second-order rule (convops), exactly as for the scaling regulariser.
"""
from __future__ import annotations

import torch

from . import convops, ops
from .gan import HeadModel


class WGAN_GP(HeadModel):
    """wgan_gp.py:4-31: d_loss = mean(D(G)) - mean(D(images)) + gp * penalty,
    g_loss = -mean(D(G)); penalty = mean((slopes - 1)^2) over the pixels of
    interpolates real + alpha (fake - real), slopes the norm over axis 1 of
    d D(x_hat) / d x_hat -- the channel axis of the reference's NCHW tensors
    (wgan_gp.py:18, as model.py:341 for the witness penalty)."""

    def __init__(self, config, **kw):
        super().__init__(config, **kw)
        self.optim_name = 'wgan_gp%d_loss' % int(config.gradient_penalty)

    def set_loss(self, G, images):
        self.d_loss, self.g_loss = ops.critic_head_loss(images, G, 0)      # wgan_gp.py:24-25
        self.optim_name = 'wgan_gp%d_loss' % int(self.config.gradient_penalty)
        self.add_slope_penalty()

    def add_slope_penalty(self):
        """wgan_gp.py:10-19, :26-27; a generator update adds none (it is a
        constant of the generator)."""
        if self.config.gradient_penalty <= 0 or not self._need_critic_grad:
            return
        bs = min(self.images.shape[0], self.G.shape[0])
        alpha = self.sample_alpha(bs)
        x_hat_data = ops.gp_interpolate(self.images[:bs].detach(), self.G[:bs].detach(), alpha,
                                        0).requires_grad_(True)
        x_hat = self.discriminator(x_hat_data)
        with convops.input_grad_only():       # no weight-gradient kernels in this pass
            g, = torch.autograd.grad(x_hat, x_hat_data, grad_outputs=ops.grad_seed(x_hat),
                                     create_graph=True)
        self.d_loss = self.d_loss + self.gp * ops.slope_penalty(g, 0.0)


__all__ = ['WGAN_GP']
