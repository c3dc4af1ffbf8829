"""One Sobolev GAN critic update and one generator update on the GPU against
float64, by the method and with the bounds of tests/test_gpu_gan_models.py: a
double deep copy of the critic on the CPU, the same images and generated
batch, and sobolevgan_gp.py:16-41 written out with create_graph=True (the decay
split as gan/core/sobolevgan_gp.py states it).

The 0.02-scale initialisation gives input gradients of about 1e-3 (c = -1
whatever the critic does), so every critic parameter is multiplied by a factor
first.  A float64 sweep on the CPU (batch 8, these seeds, uniform images) gave
c = 1.65, 3.06, 5.10 and 8.03 at 4.6, 4.8, 5.0 and 5.2 for the dcgan critic
(width 16, 32x32: the energies grow as factor^10) and c = 0.81, 3.23 and 8.62
at 1.9, 2.0 and 2.1 for resnet5 (width 64, 64x64: factor^17).  The test asserts
on its reference that c is neither within 0.05 of 0 nor above 10.

The multiplier after the step is lam + gp c: its bound is the head test's bound
on c, 1e-5 (e_r + e_f) / 2, carried through gp.
"""
import copy
import os
import sys

import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

ARCHS = {'resnet5': dict(output_size=64, df_dim=64, gf_dim=64),
         'dcgan': dict(output_size=32, df_dim=16, gf_dim=16)}
FACTORS = {'resnet5': 1.9, 'dcgan': 4.6}
LAM, GP = 0.25, 10.0


def _reference(D, x, y):
    from gan.core import snops
    params = [p for p in D.parameters() if p.requires_grad]
    final = [m for m in D.modules() if isinstance(m, snops.Linear)][-1]
    linear = {id(final.weight), id(final.bias)}
    x, y = x.requires_grad_(True), y.requires_grad_(True)
    dI, dG = D(x), D(y)
    gr, gf = torch.autograd.grad(dI.sum() + dG.sum(), (x, y), create_graph=True)    # :16-17
    e_r, e_f = (gr * gr).sum() / x.shape[0], (gf * gf).sum() / y.shape[0]            # :19-20
    c = 0.5 * e_r + 0.5 * e_f - 1.0                                                  # :22
    decay = sum((1e-3 if id(p) in linear else 1e-6) * (p * p).sum() for p in params)
    d_loss = dG.mean() - dI.mean() + LAM * c + 0.5 * GP * c * c + decay              # :29, :40-41
    grads = torch.autograd.grad(d_loss, params)
    return (float(d_loss.detach()), [g.detach() for g in grads], float(c.detach()),
            float(e_r.detach()), float(e_f.detach()))


@pytest.mark.parametrize('arch', sorted(ARCHS))
def test_sobolev_updates_match_float64(dev, arch):
    from gan.core.smmd import get_model
    from test_gpu_gan_models import _cfg, _compare, _critic_step
    torch.manual_seed(0)
    model = get_model('sobolev_gan')(_cfg(model='sobolev_gan', architecture=arch,
                                          gradient_penalty=GP, **ARCHS[arch]), device=dev)
    assert model.config.dof_dim == 1 and not model.sn_D.entries
    with torch.no_grad():
        for p in model.d_vars:
            p.mul_(FACTORS[arch])
    size = model.output_size
    g = torch.Generator().manual_seed(1)
    images = torch.rand(8, 3, size, size, generator=g).to(dev)
    z = torch.empty(8, model.z_dim).uniform_(-1, 1, generator=g).to(dev)
    model.sample_z = lambda n: z
    with torch.no_grad():
        fake = model.generator(z)
    D = copy.deepcopy(model.discriminator).double().cpu()
    ref_loss, ref_grads, c, e_r, e_f = _reference(D, images.double().cpu(), fake.double().cpu())
    print('c %.6g (e_r %.6g, e_f %.6g)' % (c, e_r, e_f))
    assert 0.05 <= abs(c) <= 10.0
    model.lam.fill_(LAM)
    got_loss, got_grads = _critic_step(model, images)
    _compare(got_loss, got_grads, ref_loss, ref_grads)
    assert model.optim_name == 'sobolevgan10_loss'
    lam = float(model.lam.double().cpu())
    tol = GP * 1e-5 * 0.5 * (e_r + e_f)
    print('lam %.9g, reference %.9g, error %.3g, bound %.3g' % (lam, LAM + GP * c,
                                                             abs(lam - (LAM + GP * c)), tol))
    assert abs(lam - (LAM + GP * c)) <= tol
    # a generator update moves neither the multiplier nor the critic
    before, lam_t = model.d_optim.flat_param.clone(), model.lam.clone()
    model.g_step(images)
    assert torch.equal(model.lam, lam_t) and torch.equal(model.d_optim.flat_param, before)


def test_flag_resolves_to_the_class():
    from gan.core.sobolevgan_gp import SobolevGAN
    from gan.main import make_flags, resolve_model
    assert resolve_model(make_flags(argv=['-model', 'sobolev_gan']).model) is SobolevGAN
