"""Sobolev GAN (gan/core/sobolevgan_gp.py) on the HIP loss kernels.

A critic update: the two critic calls on leaf copies of the real and the
generated batch, one input-gradient pass over both (create_graph), the head
(one launch: both energies, the constraint c, the augmented-Lagrangian term
and the next multiplier), the weight decay over the optimizer's flat parameter
buffer (one launch), their backwards (one launch each), the optimizer step,
and a device-side copy of the multiplier.  The rest of d_loss's gradient,
d g / d theta, is the convolutions' own second-order rule (convops), exactly
as for the scaling regulariser.

The reference leaves three things open; this build decides them:

1. The switch.  sobolevgan_gp.py:39 guards the constraint and the decay with
   ``config.sobolev_gan``, a flag the reference's main.py never defines.
   ``-model sobolev_gan`` always applies both; there is no such flag here.
2. Which parameters decay with which coefficient.  sobolevgan_gp.py:32-35
   gives 1e-3 ("linear") to the last two trainable variables of the critic
   scope, the final Linear's weight and bias, and 1e-6 ("conv") to everything
   before them, conv biases and learnable SN scales included.  Here the final
   Linear is the last ``snops.Linear`` of the critic in registration order,
   for any architecture; the decay acts on the raw stored parameters (the
   entries of ``d_optim.flat_param``), not on spectrally normalised weights.
3. The multiplier update.  sobolevgan_gp.py:42 defines ``lambda_sobolev_op``
   (lam <- lam + gp c) and nothing runs it.  Here it runs once after every
   critic update, with the c of that update's forward and no further critic
   pass: the augmented-Lagrangian step of the Sobolev GAN paper.  lam + gp c is
   also d d_loss / d c, which the head kernel has already written, so the
   update is ``lam.copy_(mult)`` on the device, with no host read-back.  ``lam``
   is a one-element device tensor, saved and restored with the model's state;
   a checkpoint without it loads as 0.  Each data-parallel tower keeps the
   multiplier of its own loss.

sobolevgan_gp.py:24 makes ``gp`` a variable; here it stays MMD_GAN's host
float.
"""
from __future__ import annotations

import torch

from . import convops, ops, snops
from .gan import HeadModel

DECAY_CONV = 1.0e-6              # sobolevgan_gp.py:37
DECAY_LINEAR = 1.0e-3            # sobolevgan_gp.py:36


def decay_table(discriminator, d_optim):
    """The decay's segments over ``d_optim.flat_param`` as host lists
    (offsets [nseg + 1], coefs [nseg]): DECAY_LINEAR for the weight and bias of
    the critic's last snops.Linear, DECAY_CONV for every other tensor of the
    optimizer, neighbours of one coefficient merged.  The segments cover the
    buffer exactly once (a tensor's segment includes its padding, which stays
    zero)."""
    linears = [m for m in discriminator.modules() if isinstance(m, snops.Linear)]
    if not linears:
        raise ValueError('the critic has no snops.Linear: no final layer to give the linear decay')
    final = {id(t) for t in (linears[-1].weight, linears[-1].bias) if t is not None}
    if not final <= {id(p) for p in d_optim.params}:
        raise ValueError("the final Linear's parameters are not in the critic's optimizer")
    offsets, coefs = [0], []
    for i, p in enumerate(d_optim.params):
        cf = DECAY_LINEAR if id(p) in final else DECAY_CONV
        if coefs and coefs[-1] == cf:
            offsets[-1] = d_optim.offsets[i + 1]
        else:
            coefs.append(cf)
            offsets.append(d_optim.offsets[i + 1])
    return offsets, coefs


class SobolevGAN(HeadModel):
    """sobolevgan_gp.py:4-46: d_loss = mean(D(G)) - mean(D(images)) + lam c +
    gp c^2 / 2 + 1e-6 sum_conv |theta|^2 + 1e-3 sum_linear |theta|^2, g_loss =
    -mean(D(G)); c = E|d D(x) / d x|^2 / 2 over the real batch + the same over
    the generated batch - 1, the squared norm over all of a sample's c, h, w
    (:19-22).  The module docstring states what the reference leaves open."""

    def __init__(self, config, **kw):
        super().__init__(config, **kw)
        self.optim_name = 'sobolevgan%d_loss' % int(config.gradient_penalty)
        self.lam = torch.zeros(1, device=self.device, dtype=torch.float32)   # sobolevgan_gp.py:27
        offsets, coefs = decay_table(self.discriminator, self.d_optim)
        self._decay_offsets = torch.tensor(offsets, dtype=torch.int64, device=self.device)
        self._decay_coefs = torch.tensor(coefs, dtype=torch.float32, device=self.device)
        self._mult = None

    # The decay hands every critic parameter, SN weights included, a gradient
    # of its own through autograd.  The SN bank's direct writers (the G-direct
    # update, the data-parallel groups' writes into the flat gradient) form an
    # SN weight's whole gradient themselves and would drop it: this model keeps
    # the bank's plain autograd node.
    def _gdirect(self):
        return False

    def _group_sn(self, bank, opt):
        return

    def set_tower_loss(self, images, fake, need_critic_grad, labels=None, fake_labels=None):
        """A critic update differentiates the critic outputs with respect to
        both batches: each becomes a leaf that requires grad (the generated
        batch keeps its graph where it has one, the reference schedule)."""
        if need_critic_grad:
            if images.dim() == 4:
                images = images.contiguous(memory_format=self.memory_format)
            images = images.detach().requires_grad_(True)
            if not fake.requires_grad:
                fake = fake.detach().requires_grad_(True)
        return super().set_tower_loss(images, fake, need_critic_grad, labels, fake_labels)

    def set_loss(self, G, images):
        self.optim_name = 'sobolevgan%d_loss' % int(self.config.gradient_penalty)
        self._mult = None
        if not self._need_critic_grad:
            # a generator update: the constraint, the decay and the multiplier
            # are constants of the generator
            self.d_loss, self.g_loss = ops.critic_head_loss(images, G, 0)  # sobolevgan_gp.py:29-30
            return
        with convops.input_grad_only():       # no weight-gradient kernels in this pass
            g_real, g_fake = torch.autograd.grad(
                [images, G], [self.images, self.G],
                grad_outputs=[ops.grad_seed(images), ops.grad_seed(G)],
                create_graph=True)                                         # sobolevgan_gp.py:16-17
        d_base, self.g_loss, self.constraint, self._mult = ops.sobolev_head_loss(
            images, G, g_real, g_fake, self.lam, self.gp)                  # :19-22, :29-30, :40
        if self.schedule == 'reference':      # this schedule also differentiates g_loss
            self.g_loss = ops.critic_head_loss(images, G, 0)[1]
        opt = self.d_optim
        self.d_loss = d_base + ops.weight_decay(opt.params, opt.flat_param, self._decay_offsets,
                                                self._decay_coefs)         # :32-37, :41

    def _exchange(self, opt):
        super()._exchange(opt)
        if opt is self.d_optim and self._mult is not None:
            self.lam.copy_(self._mult)                                     # sobolevgan_gp.py:42
            self._mult = None

    def state_dict(self):
        sd = super().state_dict()
        sd['lam'] = self.lam.clone()
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        if sd.get('lam') is None:
            self.lam.zero_()
        else:
            self.lam.copy_(sd['lam'])


__all__ = ['SobolevGAN', 'decay_table', 'DECAY_CONV', 'DECAY_LINEAR']
