"""The GAN, WGAN-GP and witness-penalty MMD critic updates on the GPU against
float64.

The float64 side is built here: a deep copy of the model's critic in double
on the CPU, the same images, the same generated batch (taken from the model's
generator and fed to both sides), the same alpha (through ``sample_alpha``),
and the reference formulas (gan/core/gan.py:10-11, gan/core/wgan_gp.py:10-27)
in plain torch with ``create_graph=True``; for ``-model mmd -gradient_penalty``
the kernel is oracle/torch_kernels.py and the penalty model.py:327-350 written
out.  Bounds are those of
tests/test_gpu_model.py for batch < 64: d_loss rtol 1e-3; per tensor
|d| <= max(2e-3 max|ref|, 5e-5 gmax) + 2e-3 |ref|; relative Frobenius error
<= 1e-3 for tensors above the noise floor.
"""
import argparse
import copy

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

# The 0.02-scale initialisation gives per-pixel slopes of about 1e-3 (a penalty
# of ~1 whatever the gradient does).  Every critic parameter is multiplied by
# this factor first; a float64 sweep on the CPU gave, for resnet5 at width 64
# and this seed, 12 % of the slopes under 0.5 and 20 % over 1.5 at 3.05 (the
# slopes double every +0.25).  The test asserts that spread on its reference.
WGAN_FACTOR = 3.05
GAN_FACTOR = 6.0          # dcgan width 16: |D(x)| about 1, inside softplus's bend


def _cfg(**kw):
    from gan.main import default_flags
    c = default_flags()
    c.update(dict(batch_size=8, kernel='rbf', batch_norm=False, with_sn=False,
                  with_scaling=False, dof_dim=1, learning_rate=1e-4, dataset='celebA'))
    c.update(kw)
    return argparse.Namespace(**c)


def _softplus64(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def _build(name, dev, factor, cl=False, near_fake=0.0, **kw):
    from gan.core.smmd import get_model
    torch.manual_seed(0)
    model = get_model(name)(_cfg(model=name, **kw), device=dev, channels_last=cl)
    with torch.no_grad():
        for p in model.d_vars:
            p.mul_(factor)
    size = model.output_size
    g = torch.Generator().manual_seed(1)
    images = torch.rand(8, 3, size, size, generator=g).to(dev)
    z = torch.empty(8, model.z_dim).uniform_(-1, 1, generator=g).to(dev)
    alpha = torch.rand(8, 1, 1, 1, generator=g).to(dev)
    model.sample_z = lambda n: z
    model.sample_alpha = lambda n: alpha[:n]
    with torch.no_grad():
        fake = model.generator(z)
    if near_fake:
        # a real batch near the generated one: the two critic passes of the
        # Wasserstein term then nearly cancel and leave the penalty visible
        noise = torch.randn(fake.shape, generator=g).to(dev)
        images = (fake + near_fake * noise).clamp(0.0, 1.0)
    return model, images, fake, alpha


_REFS = {}


def _reference(key, model, images, fake, alpha, gp):
    """(d_loss, [gradient per critic parameter], slopes) in float64 on the
    CPU; computed once per configuration (the memory format does not change
    the values) and left unchanged."""
    if key in _REFS:
        return _REFS[key]
    D = copy.deepcopy(model.discriminator).double().cpu()
    params = [p for p in D.parameters() if p.requires_grad]
    x, y, a = (t.detach().double().cpu().contiguous() for t in (images, fake, alpha))
    dI, dG = D(x), D(y)
    slopes = None
    if key[0] == 'gan':
        d_loss = (_softplus64(-dI) + _softplus64(dG)).mean()            # gan.py:10
    else:
        d_loss = dG.mean() - dI.mean()                                  # wgan_gp.py:24
        if gp > 0:
            xh = (x + a * (y - x)).requires_grad_(True)                 # wgan_gp.py:13-14
            grad, = torch.autograd.grad(D(xh).sum(), xh, create_graph=True)
            slopes = torch.sqrt((grad * grad).sum(1))                   # wgan_gp.py:18
            d_loss = d_loss + gp * ((slopes - 1.0) ** 2).mean()
    grads = torch.autograd.grad(d_loss, params, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g.detach() for g, p in zip(grads, params)]
    _REFS[key] = (float(d_loss.detach()), grads, None if slopes is None else slopes.detach())
    return _REFS[key]


def _critic_step(model, images):
    """One d_step; returns (d_loss, the gradient per critic parameter as the
    optimizer saw it), captured as tests/test_gpu_model.py does."""
    captured = {}
    orig = model.d_optim.step

    def cap(*a, **k):
        captured['g'] = model.d_optim.dense_grad().cpu()
        return orig(*a, **k)
    model.d_optim.step = cap
    model.step = 25
    model.d_counter, model.g_counter = 0, 0
    shapes = [(p.shape, p.stride()) for p in model.d_vars]
    _, d_loss, _ = model.d_step(images)
    flat = captured['g']
    grads = [torch.as_strided(flat, sh, st, model.d_optim.offsets[i]).contiguous()
             for i, (sh, st) in enumerate(shapes)]
    return float(d_loss.detach()), grads


def _tolerances(ref_grads):
    gmax = max(float(g.abs().max()) for g in ref_grads)
    return [max(2e-3 * float(g.abs().max()), 5e-5 * gmax) + 2e-3 * g.abs().numpy()
            for g in ref_grads], gmax


def _compare(got_loss, got_grads, ref_loss, ref_grads):
    assert got_loss == pytest.approx(ref_loss, rel=1e-3, abs=1e-6)
    tols, gmax = _tolerances(ref_grads)
    assert len(got_grads) == len(ref_grads)
    for i, (got, ref, tol) in enumerate(zip(got_grads, ref_grads, tols)):
        got, ref = got.numpy().astype(np.float64), ref.numpy()
        assert got.shape == ref.shape
        err = np.abs(got - ref)
        print('tensor %d %s: max err %.3g, max ref %.3g' % (i, got.shape, err.max(),
                                                          np.abs(ref).max()))
        assert (err <= tol + 1e-12).all(), (i, err.max(), np.abs(ref).max())
        if np.abs(ref).max() > 10 * 5e-5 * gmax:
            rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            assert rel <= 1e-3, (i, rel)


WGAN_KW = dict(architecture='resnet5', output_size=64, df_dim=64, gf_dim=64)


@pytest.mark.parametrize('cl', [False, True], ids=['nchw', 'nhwc'])
def test_wgan_gp_critic_step_matches_float64(dev, cl):
    model, images, fake, alpha = _build('wgan_gp', dev, WGAN_FACTOR, cl=cl, gradient_penalty=10.0,
                                        **WGAN_KW)
    assert not model.sn_D.entries                     # resnet5's critic has no SN layers
    ref_loss, ref_grads, slopes = _reference(('wgan_gp', 10.0), model, images, fake, alpha, 10.0)
    # the penalty is not trivially ~1: slopes on both sides of 1
    assert float((slopes < 0.5).double().mean()) >= 0.10
    assert float((slopes > 1.5).double().mean()) >= 0.10
    got_loss, got_grads = _critic_step(model, images)
    _compare(got_loss, got_grads, ref_loss, ref_grads)
    assert model.optim_name == 'wgan_gp10_loss'


def test_wgan_gp_penalty_matters(dev):
    """A dropped penalty cannot pass: at these inputs the penalised step and
    the gradient_penalty=0 step each meet every bound against their own
    float64 reference, and the gp = 0 gradient differs from the penalised
    reference by more than 10x the tolerance in a convolution weight.

    The real batch here is fake + 0.1 N(0, 1) (clamped to [0, 1]), not the
    uniform noise of the comparison above.  With uniform images the
    Wasserstein term is ~200x the penalty in every tensor: in float64 the
    penalty's gradient (gp = 10, penalty 0.276) is 0.2 - 0.9 % of each
    convolution weight gradient's maximum (0.62 against 109 in the input conv
    ... 0.044 against 8.4) while 10x the tolerance is 2 %, so no gp = 0 step
    can differ that much there.  Near the generated batch the two critic
    passes nearly cancel; a float64 sweep gave the penalty 2.0x and 1.2x the
    tenfold tolerance in the last block's 3x3 and 1x1 weights.

    Channels-last: in NCHW the input conv's weight gradient carries an
    absolute error of about 0.045 with or without the penalty (0.0445 on
    uniform images, 0.0483 here; channels-last 0.0067 and 0.0028), inside the
    bounds at max|ref| 109 but 1.10e-3 relative Frobenius against 1e-3 at this
    batch's max|ref| 37.6."""
    kw = dict(WGAN_KW, near_fake=0.1, cl=True)
    model, images, fake, alpha = _build('wgan_gp', dev, WGAN_FACTOR, gradient_penalty=10.0, **kw)
    ref_loss, ref_grads, slopes = _reference(('wgan_gp', 10.0, 'near'), model, images, fake,
                                             alpha, 10.0)
    assert float((slopes < 0.5).double().mean()) >= 0.10
    assert float((slopes > 1.5).double().mean()) >= 0.10
    pen_loss, pen_grads = _critic_step(model, images)
    _compare(pen_loss, pen_grads, ref_loss, ref_grads)
    plain, images0, fake0, alpha0 = _build('wgan_gp', dev, WGAN_FACTOR, gradient_penalty=0.0,
                                           **kw)
    assert torch.equal(images0, images) and torch.equal(fake0, fake)
    ref0_loss, ref0_grads, _ = _reference(('wgan_gp', 0.0, 'near'), plain, images0, fake0,
                                          alpha0, 0.0)
    got_loss, got_grads = _critic_step(plain, images0)
    _compare(got_loss, got_grads, ref0_loss, ref0_grads)       # the plain step is right too
    tols, _ = _tolerances(ref_grads)
    far = [i for i, (g0, ref, tol) in enumerate(zip(got_grads, ref_grads, tols))
           if ref.dim() == 4 and (np.abs(g0.numpy() - ref.numpy()) > 10 * tol).any()]
    print('tensors where the penalty exceeds 10x the tolerance:', far)
    assert far, 'the penalty changes no convolution weight gradient beyond the tolerance'


# -model mmd -gradient_penalty 1 -dof_dim 16: the witness penalty (model.py:327-350).
# A float64 sweep on the CPU (dcgan critic, width 16, 32x32, this seed, uniform
# images) of the factor every critic parameter is multiplied by:
#   mix_rq_1dot  the witness slopes (channel norm of d sum(witness)/d x_hat per
#                pixel) have median 0.003 at 1, 0.11 at 5, 1.0 at 6.5, 2.1 at 7
#                and 7.7 at 8; at 7.0, 5 % lie under 0.5 and 67 % over 1.5, and
#                the penalty moves every convolution weight gradient by 1.4 -
#                1.9 x the tenfold tolerance (0.4 - 0.5 x at 6.5)
#   rbf          exp(-|.|^2 / 2) saturates before the slopes grow (median 0.026
#                at 5, mmd2 = 1 from 6 on): the penalty value stays near 1, but
#                at 5.0 its gradient is 3.6 - 11.8 x the tenfold tolerance of
#                each convolution weight, against an mmd2 of 0.88
MMD_GP_FACTOR = {'mix_rq_1dot': 7.0, 'rbf': 5.0}
MMD_GP_KW = dict(architecture='dcgan', output_size=32, df_dim=16, gf_dim=16, dof_dim=16)


def _mmd_reference(key, model, images, fake, alpha, kernel, gp):
    """(d_loss, [gradient per critic parameter], slopes) of MMD_GAN.set_loss
    in float64 on the CPU: mmd2 of the kernel matrices (mmd.py:194-220) and
    model.py:327-350 written out -- interpolates, witness row means, gradient
    with create_graph, safer_norm over the channel axis, mean((. - 1)^2)."""
    if key in _REFS:
        return _REFS[key]
    from oracle import smmd_oracle as O
    from oracle.torch_kernels import kernel_xy
    D = copy.deepcopy(model.discriminator).double().cpu()
    params = [p for p in D.parameters() if p.requires_grad]
    x, y, a = (t.detach().double().cpu().contiguous() for t in (images, fake, alpha))
    spec = O.kernel_spec(kernel)
    dI, dG = D(x), D(y)
    g_loss = O.mmd2_from_K(kernel_xy(spec, dG, dG), kernel_xy(spec, dG, dI),
                           kernel_xy(spec, dI, dI), spec.const_diag)         # model.py:313-317
    d_loss = -g_loss
    slopes = None
    if gp > 0:
        xh = ((1.0 - a) * x + a * y).requires_grad_(True)                   # model.py:331-333
        hx = D(xh)
        witness = kernel_xy(spec, hx, dI).mean(1) - kernel_xy(spec, hx, dG).mean(1)
        grad, = torch.autograd.grad(witness.sum(), xh, create_graph=True)    # model.py:339
        slopes = torch.sqrt((grad * grad).sum(1) + 1.0e-5)                   # ops.py:203-206
        d_loss = d_loss + gp * ((slopes - 1.0) ** 2).mean()                  # model.py:341-344
    grads = torch.autograd.grad(d_loss, params, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g.detach() for g, p in zip(grads, params)]
    _REFS[key] = (float(d_loss.detach()), grads, None if slopes is None else slopes.detach())
    return _REFS[key]


@pytest.mark.parametrize('cl', [False, True], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('kernel', ['mix_rq_1dot', 'rbf'])
def test_mmd_witness_gp_critic_step_matches_float64(dev, kernel, cl):
    model, images, fake, alpha = _build('mmd', dev, MMD_GP_FACTOR[kernel], cl=cl, kernel=kernel,
                                        gradient_penalty=1.0, **MMD_GP_KW)
    assert not model.sn_D.entries                     # no SN, and no batch norm under a penalty
    ref_loss, ref_grads, slopes = _mmd_reference(('mmd', kernel, 1.0), model, images, fake,
                                                 alpha, kernel, 1.0)
    print('slopes: median %.3g, under 0.5 %.2f, over 1.5 %.2f' % (
        float(slopes.median()), float((slopes < 0.5).double().mean()),
        float((slopes > 1.5).double().mean())))
    if kernel == 'mix_rq_1dot':       # the penalty is not trivially ~1: slopes around and above 1
        assert 1.0 < float(slopes.median()) < 4.0
    got_loss, got_grads = _critic_step(model, images)
    _compare(got_loss, got_grads, ref_loss, ref_grads)
    assert model.optim_name == 'kernel_loss_(gp 1.0)'


@pytest.mark.parametrize('kernel', ['mix_rq_1dot', 'rbf'])
def test_mmd_witness_gp_penalty_matters(dev, kernel):
    """A dropped or mis-signed second-order term cannot pass: the
    gradient_penalty=0 step meets every bound against its own float64
    reference and differs from the penalised reference by more than 10x the
    tolerance in a convolution weight (MMD_GP_FACTOR's sweep)."""
    kw = dict(MMD_GP_KW, kernel=kernel)
    model, images, fake, alpha = _build('mmd', dev, MMD_GP_FACTOR[kernel], gradient_penalty=1.0,
                                        **kw)
    _, ref_grads, _ = _mmd_reference(('mmd', kernel, 1.0), model, images, fake, alpha, kernel,
                                     1.0)
    plain, images0, fake0, alpha0 = _build('mmd', dev, MMD_GP_FACTOR[kernel],
                                           gradient_penalty=0.0, **kw)
    # the dcgan generator's transposed convolutions do not repeat bit for bit
    assert torch.equal(images0, images) and torch.allclose(fake0, fake, rtol=0, atol=1e-5)
    ref0_loss, ref0_grads, _ = _mmd_reference(('mmd', kernel, 0.0), plain, images0, fake0,
                                              alpha0, kernel, 0.0)
    got_loss, got_grads = _critic_step(plain, images0)
    _compare(got_loss, got_grads, ref0_loss, ref0_grads)
    assert plain.optim_name == 'kernel_loss'
    tols, _ = _tolerances(ref_grads)
    far = [i for i, (g0, ref, tol) in enumerate(zip(got_grads, ref_grads, tols))
           if ref.dim() == 4 and (np.abs(g0.numpy() - ref.numpy()) > 10 * tol).any()]
    print('tensors where the penalty exceeds 10x the tolerance:', far)
    assert far, 'the penalty changes no convolution weight gradient beyond the tolerance'


def test_gan_critic_step_matches_float64(dev):
    model, images, fake, alpha = _build('gan', dev, GAN_FACTOR, architecture='dcgan',
                                        output_size=32, df_dim=16, gf_dim=16)
    ref_loss, ref_grads, _ = _reference(('gan',), model, images, fake, alpha, 0.0)
    got_loss, got_grads = _critic_step(model, images)
    _compare(got_loss, got_grads, ref_loss, ref_grads)
    assert model.optim_name == 'gan0_loss'


def test_sngan_trains_two_cycles(dev):
    """-model gan -with_sn true on sngan 32x32: two critic + generator cycles."""
    from gan.core.smmd import get_model
    torch.manual_seed(0)
    cfg = _cfg(model='gan', architecture='sngan', output_size=32, df_dim=64, gf_dim=64,
               with_sn=True, batch_norm=True, dsteps=1, start_dsteps=1, dataset='cifar10')
    model = get_model('gan')(cfg, device=dev)
    assert model.sn_D.entries
    d0 = [p.detach().clone() for p in model.d_vars]
    g0 = [p.detach().clone() for p in model.g_vars]
    u0 = [e.u.detach().clone() for e in model.sn_D.entries]
    g = torch.Generator().manual_seed(2)
    kinds = []
    for _ in range(4):
        images = torch.rand(8, 3, 32, 32, generator=g).to(dev)
        g_loss, d_loss, _ = model.train_step(images)
        kinds.append(model.d_counter == 0)
        assert np.isfinite(float(g_loss)) and np.isfinite(float(d_loss))
    assert kinds == [False, True, False, True] and model.step == 2
    assert any(not torch.equal(a, b) for a, b in zip(d0, model.d_vars))
    assert any(not torch.equal(a, b) for a, b in zip(g0, model.g_vars))
    assert all(not torch.equal(a, e.u) for a, e in zip(u0, model.sn_D.entries))


@pytest.mark.parametrize('name', ['gan', 'wgan_gp'])
def test_guards(dev, name):
    from gan.core.smmd import get_model
    cls = get_model(name)
    small = dict(architecture='dcgan', output_size=32, df_dim=16, gf_dim=16)
    with pytest.raises(NotImplementedError, match=cls.__name__):
        cls(_cfg(model=name, **small), device=dev, dp_mode='global')
    model = cls(_cfg(model=name, **small), device=dev)
    with pytest.raises(NotImplementedError, match=cls.__name__):
        model.enable_graphs(True)
