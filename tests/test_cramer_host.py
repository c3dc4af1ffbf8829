"""The Cramer GAN without a GPU: the tensor-op path of its two ops against the
formulas (gan/core/cramer.py:81-96) in float64, the model class on the CPU, the
dispatch, and the new entry points' argument checks (the library loads on a
CPU-only box)."""
import ctypes
import os
import sys

import pytest

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# the oracle stands in for the optimizer's library; the small dcgan configuration
from test_gp_host import _cfg as _base_cfg, fake  # noqa: E402,F401


def _cfg(**kw):
    return _base_cfg(gradient_penalty=10.0, **kw)

EPS = 1.0e-5
CPU = torch.device('cpu')


def _n(v):
    return torch.sqrt((v * v).sum(1) + EPS)


@pytest.mark.parametrize('variant', ['cramer', 'reddit_cramer'])
def test_plain_ops_match_the_formulas(variant):
    from gan.core import ops
    gen = torch.Generator().manual_seed(0)
    g, g2, x, w = (torch.randn(5, 7, generator=gen, dtype=torch.float64) for _ in range(4))
    d_base, g_loss = ops.cramer_head_loss(g, g2, x, variant)
    if variant == 'cramer':
        ref_g = (-_n(g - g2) + _n(g - x) + _n(g2 - x)).mean()
        ref_d = (-_n(x - g) + _n(x) + _n(g2 - g) - _n(g2)).mean()
    else:
        ref_g = ((_n(x - g) - _n(x)) - (_n(g - g2) - _n(g))).mean()
        ref_d = -ref_g
    assert float(d_base) == pytest.approx(float(ref_d), rel=1e-12)
    assert float(g_loss) == pytest.approx(float(ref_g), rel=1e-12)
    # the seed and the gradient through it: P_v w = w / n(v) - v (v.w) / n(v)^3
    h = x.clone().requires_grad_(True)
    gg = g.clone().requires_grad_(True)
    U = ops.cramer_seed(h, gg)
    a = (x - g)
    assert torch.allclose(U, a / _n(a)[:, None] - x / _n(x)[:, None], rtol=1e-12, atol=0)
    gH, gG = torch.autograd.grad((U * w).sum(), (h, gg))

    def P(v):
        return w / _n(v)[:, None] - v * (v * w).sum(1, keepdim=True) / _n(v)[:, None] ** 3
    assert torch.allclose(gH, P(a) - P(x), rtol=1e-10, atol=1e-14)
    assert torch.allclose(gG, -P(a), rtol=1e-10, atol=1e-14)
    with pytest.raises(ValueError):
        ops.cramer_head_loss(g, g2[:4], x, variant)
    with pytest.raises(ValueError):
        ops.cramer_seed(x[:4], g)


@pytest.mark.parametrize('name', ['cramer', 'reddit_cramer'])
def test_model_on_the_cpu(fake, name):  # noqa: F811
    from gan.core.cramer import Cramer_GAN
    from gan.main import resolve_model
    assert resolve_model(name) is Cramer_GAN
    torch.manual_seed(0)
    m = Cramer_GAN(_cfg(model=name), device=CPU)
    assert m.config.dof_dim == 4 and m.discriminator(torch.zeros(2, 3, 16, 16)).shape == (2, 4)
    assert m.optim_name == '%s gp 10.0' % name
    # z is drawn before z2, both through sample_z
    zs = [torch.full((6, m.z_dim), 0.25), torch.full((6, m.z_dim), -0.5)]
    drawn = []
    m.sample_z = lambda n: (drawn.append(len(drawn)), zs[len(drawn) - 1])[1]
    with torch.no_grad():
        fake_b, _ = m._generate(6)
        assert drawn == [0, 1]
        assert torch.equal(fake_b, m.generator(zs[0]))
        assert torch.equal(m._G2_next, m.generator(zs[1]))
    # a critic loss with the penalty: finite, differentiable into every critic tensor
    images = torch.rand(6, 3, 16, 16)
    g_loss, d_loss, _ = m.set_tower_loss(images, fake_b, need_critic_grad=True)
    assert m.d_G2.shape == (6, 4) and m.G2.shape == fake_b.shape
    grads = torch.autograd.grad(d_loss, m.d_vars, allow_unused=True)
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    _, base, _ = m.set_tower_loss(images, fake_b, need_critic_grad=False, fake2=m.G2)
    assert float(base.detach()) != float(d_loss.detach())     # a generator step adds no penalty


def test_guards_and_wrong_model(fake):  # noqa: F811
    from gan.core.cramer import Cramer_GAN
    with pytest.raises(NotImplementedError, match='Cramer_GAN'):
        Cramer_GAN(_cfg(model='cramer'), device=CPU, dp_mode='global')
    m = Cramer_GAN(_cfg(model='cramer'), device=CPU)
    with pytest.raises(NotImplementedError, match='Cramer_GAN'):
        m.enable_graphs(True)
    m.enable_graphs(False)
    with pytest.raises(AttributeError, match='wrong model'):
        Cramer_GAN(_cfg(model='wgan_gp'), device=CPU)


def test_library_argument_checks():
    from gan.core import _lib
    L = _lib.lib()
    x = ctypes.c_void_p(4096)      # never dereferenced: every call is refused before a launch
    big = 1 << 20
    assert L.smmd_cramer_head_workspace_bytes(0, 4) == 0
    assert L.smmd_cramer_head_workspace_bytes(70, 16) >= 256 + 5 * 2 * 8

    def head(G=x, G2=x, X=x, b=4, d=8, variant=0, eps=1e-5, want=3, out=x, gd=(x, x, x),
             gg=(x, x, x), ws=x, nb=big):
        return L.smmd_cramer_head_fwd(G, G2, X, b, d, variant, eps, want, out, *gd, *gg, ws, nb,
                                      None)
    bad = [dict(G=None), dict(G2=None), dict(X=None), dict(out=None), dict(b=0), dict(d=0),
           dict(variant=2), dict(variant=-1), dict(want=0), dict(want=4), dict(eps=-1.0),
           dict(gd=(x, None, x)), dict(gg=(None, x, x)), dict(want=1, gd=(None, None, None))]
    for kw in bad:
        assert head(**kw) == 1, kw
    assert head(ws=None) == 3 and head(nb=8) == 3
    n = ctypes.c_void_p(8192)
    for args in ((None, x, 4, 8, 1e-5, x, n), (x, None, 4, 8, 1e-5, x, n),
                 (x, x, 4, 8, 1e-5, None, n), (x, x, 4, 8, 1e-5, x, None),
                 (x, x, 0, 8, 1e-5, x, n), (x, x, 4, 0, 1e-5, x, n), (x, x, 4, 8, -1.0, x, n)):
        assert L.smmd_cramer_seed_fwd(*args, None) == 1, args
    for args in ((None, x, n, x, 4, 8, x, x), (x, None, n, x, 4, 8, x, x),
                 (x, x, None, x, 4, 8, x, x), (x, x, n, None, 4, 8, x, x),
                 (x, x, n, x, 4, 8, None, x), (x, x, n, x, 4, 8, x, None),
                 (x, x, n, x, 0, 8, x, x), (x, x, n, x, 4, 0, x, x)):
        assert L.smmd_cramer_seed_bwd(*args, None) == 1, args
