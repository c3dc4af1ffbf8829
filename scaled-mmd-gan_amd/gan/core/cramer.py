"""The Cramer GAN (gan/core/cramer.py) on the HIP loss kernels.

A step draws two generated batches.  A critic update: three critic calls
(real, G, G2), the energy-distance head (one launch: both losses and the row
gradients of the one being applied), then the penalty -- interpolates (one
launch), a fourth critic call, the seed d to_penalize / d D(x_hat) (one
launch), one input-gradient pass seeded with it, the per-pixel slopes and
their penalty (one launch forward, one backward).  The seed depends on the
critic, so the penalty's gradient also flows back through it (one launch,
ops.cramer_seed's backward) on top of the convolutions' own second-order rule.
"""
from __future__ import annotations

import torch

from . import convops, ops
from .mmd import _eps
from .model import MMD_GAN


class Cramer_GAN(MMD_GAN):
    """cramer.py:6-107.  ``config.model`` selects the loss: 'cramer'
    (cramer.py:85-88, the Cramer GAN paper) or 'reddit_cramer' (:90-92); both
    penalise critic(x_hat, G) = n(D(x_hat) - D(G)) - n(D(x_hat)) (:88, :92, :96-102).
    dof_dim is the configuration's (the paper uses 256); no scaling
    regulariser; tower-mode data parallel only, no step graphs."""

    def __init__(self, config, device=None, process_group=None, dp_mode='tower', **kw):
        if dp_mode == 'global':
            raise NotImplementedError(
                "%s: dp_mode='global' is not built for this model (its loss pairs the rows of "
                "the local batches; use dp_mode='tower')" % type(self).__name__)
        self._variant(config)
        if getattr(config, 'with_labels', False):
            raise NotImplementedError('%s: the conditional pair is not built for this model'
                                      % type(self).__name__)
        super().__init__(config, device=device, process_group=process_group, dp_mode=dp_mode,
                         **kw)
        self.G2 = self.d_G2 = self._G2_next = None
        self.optim_name = '%s gp %.1f' % (config.model, config.gradient_penalty)

    @staticmethod
    def _variant(config):
        if config.model not in ops.CRAMER_VARIANTS:
            raise AttributeError('wrong model: %s' % config.model)          # cramer.py:94
        return config.model

    def _scaling_ahead(self):
        return False                 # cramer.py never calls add_scaling

    def enable_graphs(self, on=True):
        if on:
            raise NotImplementedError(
                '%s: step graphs are not built for this model (the penalty\'s critic call and '
                'its alpha draw are unproven under capture)' % type(self).__name__)
        super().enable_graphs(False)

    def _generate(self, n):
        """G(z) and, kept for the step's set_tower_loss, G2 = G(z2): z first,
        z2 second, in the caller's grad mode (cramer.py:33-48)."""
        z = self.sample_z(n)
        z2 = self.sample_z(n)
        fake = self.generator(z)
        self._G2_next = self.generator(z2)
        return fake, None

    @torch.no_grad()
    def get_samples(self, n):
        out, have = [], 0
        while have < n:
            out.append(self.generator(self.sample_z(self.batch_size)))
            have += out[-1].shape[0]
        return torch.cat(out)[:n]

    def set_tower_loss(self, images, fake, need_critic_grad, labels=None, fake_labels=None,
                       fake2=None):
        """cramer.py:51-57: the critic on the real batch and on both generated
        batches, then ``set_loss(d_G, d_G2, d_images)``.  ``fake2``: the
        second generated batch (default: the one the step's ``_generate``
        drew with ``fake``)."""
        if labels is not None or fake_labels is not None:
            raise ValueError('labels given to a model built without with_labels')
        if fake2 is None:
            fake2, self._G2_next = self._G2_next, None
        if fake2 is None:
            raise ValueError('%s needs a second generated batch (fake2)' % type(self).__name__)
        D = self.discriminator
        if images.dim() == 4:
            images = images.contiguous(memory_format=self.memory_format)
        self.images = self._last_images = images
        self.G, self.G2 = fake, fake2
        self._need_critic_grad = need_critic_grad
        self.aux = None
        self.d_images_layers = self.d_G_layers = None
        self.d_images = D(images)
        self.d_G = D(fake)
        self.d_G2 = D(fake2)
        self.set_loss(self.d_G, self.d_G2, self.d_images)
        self.fused_loss = False
        return self.g_loss, self.d_loss, self.aux

    def set_loss(self, G, G2, images):
        """cramer.py:72-104."""
        c = self.config
        variant = self._variant(c)
        # the losses this step differentiates: the critic's, the generator's,
        # or (the reference schedule computes both gradient sets) both
        want = 3 if self.schedule == 'reference' else (1 if self._need_critic_grad else 2)
        self.d_loss, self.g_loss = ops.cramer_head_loss(G, G2, images, variant, _eps, want=want)
        self.optim_name = '%s gp %.1f' % (c.model, c.gradient_penalty)
        if c.gradient_penalty <= 0 or not self._need_critic_grad:
            return                   # a constant of the generator, as in WGAN_GP
        bs = min(self.images.shape[0], self.G.shape[0])
        alpha = self.sample_alpha(bs)
        x_hat_data = ops.gp_interpolate(self.images[:bs].detach(), self.G[:bs].detach(), alpha,
                                        1).requires_grad_(True)                 # cramer.py:78
        x_hat = self.discriminator(x_hat_data)
        seed = ops.cramer_seed(x_hat, G[:bs], _eps)                             # cramer.py:88, :96
        with convops.input_grad_only():       # no weight-gradient kernels in this pass
            grad, = torch.autograd.grad(x_hat, x_hat_data, grad_outputs=seed, create_graph=True)
        self.d_loss = self.d_loss + self.gp * ops.slope_penalty(grad, _eps)     # cramer.py:98-102

    def _detach_step_state(self):
        for name in ('G2', 'd_G2'):
            v = getattr(self, name, None)
            if torch.is_tensor(v):
                setattr(self, name, v.detach())
        self._G2_next = None
        return super()._detach_step_state()


__all__ = ['Cramer_GAN']
