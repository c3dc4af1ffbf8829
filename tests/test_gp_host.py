"""The GAN and WGAN-GP baselines without a GPU: the model dispatch, the new
entry points' argument checks (the library loads on a CPU-only box), and the
two models' losses on the CPU -- where the ops take their plain-tensor path --
against the reference formulas (gan/core/gan.py:10-11,
gan/core/wgan_gp.py:10-27) evaluated here in float64."""
import argparse
import copy
import ctypes
import os
import sys

import pytest

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


@pytest.fixture
def fake(monkeypatch):
    """The oracle stands in for the library where a CPU model needs it (the
    optimizer, the SN bank), as in tests/test_model_hooks.py; the new ops take
    their plain-tensor path on CPU tensors and never reach it."""
    import fake_lib
    from gan.core import _lib
    f = fake_lib.FakeLib()
    monkeypatch.setattr(_lib, '_lib', f)
    monkeypatch.setattr(_lib, 'lib', lambda: f)
    monkeypatch.setattr(_lib, 'require_cuda', lambda *t: None)
    monkeypatch.setattr(_lib, 'stream_handle', lambda device=None: None)
    monkeypatch.setattr(_lib, 'workspace', lambda tag, nbytes, device: torch.zeros(
        max(int(nbytes), 256), dtype=torch.uint8))
    return f


def _cfg(**kw):
    from gan.main import default_flags
    c = default_flags()
    c.update(dict(batch_size=6, output_size=16, architecture='dcgan', kernel='rbf',
                  batch_norm=False, with_sn=False, with_scaling=False, dof_dim=4, df_dim=4,
                  gf_dim=4, learning_rate=1e-4, dataset='cifar10'))
    c.update(kw)
    return argparse.Namespace(**c)


def test_dispatch(fake):
    from gan.core.model import MMD_GAN
    from gan.core.smmd import get_model
    for name, optim in (('gan', 'gan0_loss'), ('wgan_gp', 'wgan_gp10_loss')):
        cls = get_model(name)
        assert issubclass(cls, MMD_GAN) and cls is not MMD_GAN
        gp = 10.0 if name == 'wgan_gp' else 0.0
        m = cls(_cfg(model=name, gradient_penalty=gp), device=torch.device('cpu'))
        assert m.config.dof_dim == 1                 # forced, whatever the flag said
        assert m.discriminator(torch.zeros(2, 3, 16, 16)).shape == (2, 1)
        assert m.optim_name == optim
    with pytest.raises(NotImplementedError):
        get_model('cramer')
    with pytest.raises(ValueError):
        get_model('nope')


def test_guards_on_the_cpu(fake):
    from gan.core.smmd import get_model
    for name in ('gan', 'wgan_gp'):
        cls = get_model(name)
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(_cfg(model=name), device=torch.device('cpu'), dp_mode='global')
        m = cls(_cfg(model=name), device=torch.device('cpu'))
        with pytest.raises(NotImplementedError, match=cls.__name__):
            m.enable_graphs(True)
        m.enable_graphs(False)


def test_library_argument_checks():
    from gan.core import _lib
    L = _lib.lib()
    x = ctypes.c_void_p(4096)
    # every call below is refused before any launch (x is not a real buffer)
    # interpolates
    assert L.smmd_gp_interp(None, x, x, x, 2, 48, 0, None) == 1
    assert L.smmd_gp_interp(x, None, x, x, 2, 48, 0, None) == 1
    assert L.smmd_gp_interp(x, x, None, x, 2, 48, 0, None) == 1
    assert L.smmd_gp_interp(x, x, x, None, 2, 48, 0, None) == 1
    assert L.smmd_gp_interp(x, x, x, x, 0, 48, 0, None) == 1
    assert L.smmd_gp_interp(x, x, x, x, 2, 0, 0, None) == 1
    assert L.smmd_gp_interp(x, x, x, x, 2, 48, 2, None) == 1
    # slopes
    assert L.smmd_gp_slope_workspace_bytes(0, 3, 16) == 0
    need = L.smmd_gp_slope_workspace_bytes(8, 3, 64 * 64)
    assert need >= 8 * (8 * 64 * 64 // 1024)         # one double per 1024-pixel block
    big = 1 << 20
    assert L.smmd_gp_slope_fwd(None, 8, 3, 4096, 0, 0.0, x, x, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 8, 3, 4096, 0, 0.0, None, x, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 8, 3, 4096, 0, 0.0, x, None, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 0, 3, 4096, 0, 0.0, x, x, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 8, 0, 4096, 0, 0.0, x, x, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 8, 3, 0, 0, 0.0, x, x, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 8, 3, 4096, 0, -1.0, x, x, x, big, None) == 1
    assert L.smmd_gp_slope_fwd(x, 8, 3, 4096, 0, 0.0, x, x, None, big, None) == 3
    assert L.smmd_gp_slope_fwd(x, 8, 3, 4096, 0, 0.0, x, x, x, need - 1, None) == 3
    assert L.smmd_gp_slope_fwd(x, 8, 3, 4096, 1, 0.0, x, x, x, need - 1, None) == 3
    assert L.smmd_gp_slope_bwd(None, x, 8, 3, 4096, 0, x, x, None) == 1
    assert L.smmd_gp_slope_bwd(x, None, 8, 3, 4096, 0, x, x, None) == 1
    assert L.smmd_gp_slope_bwd(x, x, 8, 3, 4096, 0, None, x, None) == 1
    assert L.smmd_gp_slope_bwd(x, x, 8, 3, 4096, 0, x, None, None) == 1
    assert L.smmd_gp_slope_bwd(x, x, 0, 3, 4096, 0, x, x, None) == 1
    assert L.smmd_gp_slope_bwd(x, x, 8, 0, 4096, 0, x, x, None) == 1
    assert L.smmd_gp_slope_bwd(x, x, 8, 3, 0, 0, x, x, None) == 1
    # head
    assert L.smmd_critic_head_fwd(None, 4, x, 4, 0, x, x, x, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, None, 4, 0, x, x, x, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, x, 4, 0, None, x, x, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, x, 4, 0, x, None, x, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, x, 4, 0, x, x, None, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, x, 4, 0, x, x, x, None, None) == 1
    assert L.smmd_critic_head_fwd(x, 0, x, 4, 0, x, x, x, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, x, 0, 1, x, x, x, x, None) == 1
    assert L.smmd_critic_head_fwd(x, 4, x, 4, 2, x, x, x, x, None) == 1


def _build(name, **kw):
    from gan.core.smmd import get_model
    torch.manual_seed(0)
    m = get_model(name)(_cfg(model=name, **kw), device=torch.device('cpu'))
    with torch.no_grad():               # the 0.02-std init gives slopes ~ 1e-7: move them
        for p in m.d_vars:
            p.mul_(20.0)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(6, 3, 16, 16, generator=g)
    z = torch.empty(6, m.z_dim).uniform_(-1, 1, generator=g)
    alpha = torch.rand(6, 1, 1, 1, generator=g)
    with torch.no_grad():
        fake = m.generator(z)
    m.sample_alpha = lambda n: alpha[:n].clone()
    return m, images, fake, alpha


def _softplus64(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def test_wgan_gp_cpu_loss_matches_float64(fake):
    m, images, fake, alpha = _build('wgan_gp', gradient_penalty=10.0)
    g_loss, d_loss, _ = m.set_tower_loss(images, fake, need_critic_grad=True)
    D = copy.deepcopy(m.discriminator).double()
    x, y, a = images.double(), fake.double(), alpha.double()
    xh = (x + a * (y - x)).requires_grad_(True)                     # wgan_gp.py:13-14
    grad, = torch.autograd.grad(D(xh).sum(), xh)
    slopes = torch.sqrt((grad * grad).sum(1))                       # wgan_gp.py:18
    pen = ((slopes - 1.0) ** 2).mean()
    assert 0.05 < float(slopes.median()) < 20.0        # neither ~0 nor blown up
    dG, dI = D(y), D(x)
    ref_d = dG.mean() - dI.mean() + 10.0 * pen
    ref_g = -dG.mean()
    assert float(d_loss.detach()) == pytest.approx(float(ref_d.detach()), rel=1e-5)
    assert float(g_loss.detach()) == pytest.approx(float(ref_g.detach()), rel=1e-5)
    # differentiable through the penalty's double backward
    grads = torch.autograd.grad(d_loss, m.d_vars, allow_unused=True)
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    # a generator step adds no penalty
    _, d_loss_g, _ = m.set_tower_loss(images, fake, need_critic_grad=False)
    assert float(d_loss_g.detach()) == pytest.approx(float((dG.mean() - dI.mean()).detach()), rel=1e-5)


def test_gan_cpu_loss_matches_float64(fake):
    m, images, fake, _ = _build('gan')
    g_loss, d_loss, _ = m.set_tower_loss(images, fake, need_critic_grad=True)
    D = copy.deepcopy(m.discriminator).double()
    dG, dI = D(fake.double()), D(images.double())
    ref_d = (_softplus64(-dI) + _softplus64(dG)).mean()             # gan.py:10
    ref_g = _softplus64(-dG).mean()                                 # gan.py:11
    assert float(d_loss.detach()) == pytest.approx(float(ref_d.detach()), rel=1e-5)
    assert float(g_loss.detach()) == pytest.approx(float(ref_g.detach()), rel=1e-5)


def test_ops_plain_path_order():
    """The plain-tensor path keeps the stated arithmetic order."""
    from gan.core import ops
    g = torch.Generator().manual_seed(3)
    real, fake = torch.randn(3, 3, 5, 7, generator=g), torch.randn(3, 3, 5, 7, generator=g)
    a = torch.rand(3, 1, 1, 1, generator=g)
    assert torch.equal(ops.gp_interpolate(real, fake, a, 0), real + a * (fake - real))
    assert torch.equal(ops.gp_interpolate(real, fake, a, 1), (1.0 - a) * real + a * fake)
    x = torch.randn(3, 3, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    p = ops.slope_penalty(x, 0.0)
    s = torch.sqrt((x * x).sum(1))
    assert float(p.detach()) == pytest.approx(float(((s - 1) ** 2).mean().detach()), rel=1e-12)
    gx, = torch.autograd.grad(p, x)
    ref = (2 * (s - 1) / (s * s.numel())).unsqueeze(1) * x
    assert torch.allclose(gx, ref.detach(), rtol=1e-10, atol=0)
