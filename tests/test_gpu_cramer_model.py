"""One Cramer GAN critic update on the GPU against float64, by the method and
with the bounds of tests/test_gpu_gan_models.py: a double deep copy of the
critic on the CPU, the same images, G, G2 and alpha (stubbed sample_z /
sample_alpha), and cramer.py:72-102 written out with create_graph=True.

The 0.02-scale initialisation gives slopes of about 1e-3 (a penalty of ~1
whatever the gradient does), so every critic parameter is multiplied by
FACTOR first.  A float64 sweep on the CPU (dcgan critic, width 16, 32x32,
dof_dim 16, this seed, uniform images; the slopes grow as factor^5) gave a
median slope of 0.35 at 7, 0.69 at 8, 0.93 at 8.5 and 1.24 at 9; at 8.5, 21 %
of the slopes lie under 0.5 and 22 % over 1.5.  The test asserts that spread
on its reference.
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

FACTOR = 8.5
EPS = 1.0e-5


def _n(v):
    return torch.sqrt((v * v).sum(1) + EPS)


def _reference(D, name, x, y, y2, a, gp):
    params = [p for p in D.parameters() if p.requires_grad]
    dI, dG, dG2 = D(x), D(y), D(y2)
    if name == 'cramer':                                                 # cramer.py:85-88
        d_loss = (-_n(dI - dG) + _n(dI) + _n(dG2 - dG) - _n(dG2)).mean()
    else:                                                                # cramer.py:90-92
        d_loss = -((_n(dI - dG) - _n(dI)) - (_n(dG - dG2) - _n(dG))).mean()
    xh = ((1.0 - a) * x + a * y).requires_grad_(True)                    # cramer.py:78
    hx = D(xh)
    grad, = torch.autograd.grad((_n(hx - dG) - _n(hx)).sum(), xh, create_graph=True)
    slopes = torch.sqrt((grad * grad).sum(1) + EPS)                      # cramer.py:98
    d_loss = d_loss + gp * ((slopes - 1.0) ** 2).mean()
    grads = torch.autograd.grad(d_loss, params)
    return float(d_loss.detach()), [g.detach() for g in grads], slopes.detach()


@pytest.mark.parametrize('name', ['cramer', 'reddit_cramer'])
def test_cramer_critic_step_matches_float64(dev, name):
    from gan.core.cramer import Cramer_GAN
    from test_gpu_gan_models import _cfg, _compare, _critic_step
    torch.manual_seed(0)
    model = Cramer_GAN(_cfg(model=name, architecture='dcgan', output_size=32, df_dim=16,
                            gf_dim=16, dof_dim=16, gradient_penalty=10.0), device=dev)
    assert model.config.dof_dim == 16 and not model.sn_D.entries
    with torch.no_grad():
        for p in model.d_vars:
            p.mul_(FACTOR)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(8, 3, 32, 32, generator=g).to(dev)
    zs = [torch.empty(8, model.z_dim).uniform_(-1, 1, generator=g).to(dev) for _ in range(2)]
    alpha = torch.rand(8, 1, 1, 1, generator=g).to(dev)
    with torch.no_grad():
        fakes = [model.generator(z) for z in zs]
    draws = iter(zs)
    model.sample_z = lambda n: next(draws)               # z first, z2 second
    model.sample_alpha = lambda n: alpha[:n]
    D = copy.deepcopy(model.discriminator).double().cpu()
    x, y, y2, a = (t.detach().double().cpu().contiguous() for t in (images, *fakes, alpha))
    ref_loss, ref_grads, slopes = _reference(D, name, x, y, y2, a, 10.0)
    print('slopes: median %.3g, under 0.5 %.2f, over 1.5 %.2f' % (
        float(slopes.median()), float((slopes < 0.5).double().mean()),
        float((slopes > 1.5).double().mean())))
    assert float((slopes < 0.5).double().mean()) >= 0.10
    assert float((slopes > 1.5).double().mean()) >= 0.10
    got_loss, got_grads = _critic_step(model, images)
    # the dcgan generator's transposed convolutions do not repeat bit for bit
    assert torch.allclose(model.G, fakes[0], rtol=0, atol=1e-5)
    assert torch.allclose(model.G2, fakes[1], rtol=0, atol=1e-5)
    assert model.d_G2.shape == (8, 16) and not model.d_G2.requires_grad
    _compare(got_loss, got_grads, ref_loss, ref_grads)
    assert model.optim_name == '%s gp 10.0' % name
