"""The class-conditional SMMD steps on the GPU against float64.

cond_snresnet, width 8 for both networks, batch 8, 64x64, 5 classes, -model
smmd with spectral normalisation and the scaling regulariser.  The float64
side is built here in plain torch on the CPU: deep copies of the model's
networks in double, each SN layer's effective weight s W / sigma from one
power iteration on the bank's u (sn.py:14-46, u and v constants of the
gradient), the rbf MMD^2 (mmd.py:55-82, :199-219) times the scale
1 / (sc mean_i ||d D(x_i) / d x_i||^2 + 1) (model.py:366-403), with the labels
of the real batch and the drawn labels of the generated one at the critic
(model.py:297-301).  Bounds are those of tests/test_gpu_gan_models.py: loss
rtol 1e-3; per tensor |d| <= max(2e-3 max|ref|, 5e-5 gmax) + 2e-3 |ref|;
relative Frobenius error <= 1e-3 for tensors above the noise floor.
"""
import argparse
import copy

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

K = 5
# Seed of the images, z and labels.  Chosen on the CPU (float64 side alone) so
# that the critic gradient with the real batch's labels rolled by one differs
# from the true one, in the embedding's gradient, by more than ten times that
# tensor's bound: see test_a_dropped_label_cannot_pass.
DATA_SEED = 2


def _cfg(**kw):
    from gan.main import default_flags
    c = default_flags()
    c.update(dict(batch_size=8, output_size=64, architecture='cond_snresnet', with_labels=True,
                  num_classes=K, kernel='rbf', model='smmd', batch_norm=True, with_sn=True,
                  with_learnable_sn_scale=True, with_scaling=True, dof_dim=2, df_dim=8, gf_dim=8,
                  learning_rate=1e-4, dataset='imagenet'))
    c.update(kw)
    return argparse.Namespace(**c)


def build(dev):
    """(model, images, labels, z, y): everything drawn on the CPU, the SN
    bank's u vectors included, so the float64 side sees the same values
    wherever the model lives."""
    from gan.core.smmd import SMMD
    torch.manual_seed(0)
    model = SMMD(_cfg(), device=dev)
    g = torch.Generator().manual_seed(DATA_SEED)
    with torch.no_grad():
        for e in model.sn_D.entries:
            u = torch.randn(e.u.shape, generator=g)
            e.u.copy_(u / u.norm())
        # trained tables are not ones and zeros: every class its own rows
        for m in model.generator.modules():
            if hasattr(m, 'offset'):
                m.scale.copy_(1.0 + 0.3 * torch.randn(m.scale.shape, generator=g))
                m.offset.copy_(0.3 * torch.randn(m.offset.shape, generator=g))
    images = torch.rand(8, 3, 64, 64, generator=g)
    labels = torch.randint(0, K, (8,), generator=g)
    z = torch.empty(8, model.z_dim).uniform_(-1, 1, generator=g)
    y = torch.randint(0, K, (8,), generator=g)
    model.sample_z = lambda n: z.to(dev)
    model.sample_y = lambda n: y.to(dev)
    return model, images, labels, z, y


def _l2n(v):
    return v / (v.norm() + 1e-12)


def mirror(model):
    """Float64 CPU copies (G, D) of the model's networks, each SN layer of D
    holding its effective weight as a function of its own W and s."""
    from gan.core.snops import sn_modules
    G = copy.deepcopy(model.generator).double().cpu()
    D = copy.deepcopy(model.discriminator).double().cpu()
    mods = sn_modules(D)
    assert len(mods) == len(model.sn_D.entries)
    for m, e in zip(mods, model.sn_D.entries):
        assert m.weight.shape == e.module.weight.shape
        W = m.weight.reshape(m.weight.shape[0], -1)
        with torch.no_grad():
            v = _l2n(e.u.detach().double().cpu() @ W)
            u = _l2n(W @ v)
        sigma = u @ W @ v
        m.w_eff = m.sn_scale * m.weight / sigma
    return G, D


def _rbf_mmd2(X, Y):
    """mmd2(_rbf_kernel(X, Y)) with sigma 1, wt 1 (const_diagonal 1)."""
    def k(A, B):
        d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.t()
        return torch.exp(-0.5 * d2.clamp(min=0.0))
    m, n = X.shape[0], Y.shape[0]
    return ((k(X, X).sum() - m) / (m * (m - 1)) + (k(Y, Y).sum() - n) / (n * (n - 1))
            - 2.0 * k(X, Y).sum() / (m * n))


def smmd64(D, images, labels, fake, y, sc, create_graph):
    """g_loss of smmd.py:11-23 in float64."""
    x = images.double().requires_grad_(True)
    dI, dG = D(x, y=labels), D(fake, y=y)
    n2 = 0.0
    for j in range(dI.shape[1]):
        gj, = torch.autograd.grad(dI[:, j].sum(), x, create_graph=create_graph, retain_graph=True)
        n2 = n2 + (gj * gj).sum((1, 2, 3))
    scale = 1.0 / (sc * n2.mean() + 1.0)
    return _rbf_mmd2(dG, dI) * scale


def critic_reference(model, images, labels, y, fake):
    _, D = mirror(model)
    params = [p for p in D.parameters() if p.requires_grad]
    g_loss = smmd64(D, images, labels, fake.double().cpu(), y, model.sc, True)
    grads = torch.autograd.grad(-g_loss, params, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g.detach() for g, p in zip(grads, params)]
    names = [n for n, p in D.named_parameters() if p.requires_grad]
    return float(-g_loss.detach()), grads, names


def generator_reference(model, images, labels, z, y):
    G, D = mirror(model)
    params = [p for p in G.parameters() if p.requires_grad]
    g_loss = smmd64(D, images, labels, G(z.double(), y), y, model.sc, False)
    grads = torch.autograd.grad(g_loss, params, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g.detach() for g, p in zip(grads, params)]
    names = [n for n, p in G.named_parameters() if p.requires_grad]
    return float(g_loss.detach()), grads, names


def tolerances(ref_grads):
    gmax = max(float(g.abs().max()) for g in ref_grads)
    return [max(2e-3 * float(g.abs().max()), 5e-5 * gmax) + 2e-3 * g.abs().numpy()
            for g in ref_grads], gmax


def _compare(got_loss, got_grads, ref_loss, ref_grads, names):
    assert got_loss == pytest.approx(ref_loss, rel=1e-3, abs=1e-6)
    tols, gmax = tolerances(ref_grads)
    assert len(got_grads) == len(ref_grads)
    for name, got, ref, tol in zip(names, got_grads, ref_grads, tols):
        got, ref = got.numpy().astype(np.float64), ref.numpy()
        assert got.shape == ref.shape
        err = np.abs(got - ref)
        print('%s %s: max err %.3g, max ref %.3g' % (name, got.shape, err.max(),
                                                    np.abs(ref).max()))
        assert (err <= tol + 1e-12).all(), (name, err.max(), np.abs(ref).max())
        if np.abs(ref).max() > 10 * 5e-5 * gmax:
            rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            assert rel <= 1e-3, (name, rel)


def _step(model, opt, params, run):
    """One step; (its result, the gradient per parameter as the optimizer saw
    it), captured as tests/test_gpu_model.py does."""
    captured = {}
    orig = opt.step

    def cap(*a, **k):
        captured['g'] = opt.dense_grad().cpu()
        return orig(*a, **k)
    opt.step = cap
    model.step = 25
    model.d_counter, model.g_counter = 0, 0
    shapes = [(p.shape, p.stride()) for p in params]
    out = run()
    flat = captured['g']
    return out, [torch.as_strided(flat, sh, st, opt.offsets[i]).contiguous()
                 for i, (sh, st) in enumerate(shapes)]


def test_critic_step_matches_float64(dev):
    model, images, labels, z, y = build(dev)
    with torch.no_grad():
        fake = model.generator(z.to(dev), y.to(dev))
    ref_loss, ref_grads, names = critic_reference(model, images, labels, y, fake)
    assert 'embed.weight' in names and 'embed.sn_scale' in names
    (_, d_loss, _), grads = _step(model, model.d_optim, model.d_vars,
                                  lambda: model.d_step(images.to(dev), labels.to(dev)))
    _compare(float(d_loss), grads, ref_loss, ref_grads, names)
    assert torch.equal(model.labels.cpu(), labels) and torch.equal(model.y.cpu(), y)


def test_generator_step_matches_float64(dev):
    model, images, labels, z, y = build(dev)
    ref_loss, ref_grads, names = generator_reference(model, images, labels, z, y)
    assert any(n.endswith('bn1.scale') for n in names)
    assert any(n.endswith('bn2.offset') for n in names)
    # the tables' gradients are there to be compared: not noise-floor tensors
    gmax = max(float(g.abs().max()) for g in ref_grads)
    for n, g in zip(names, ref_grads):
        if n.endswith(('.scale', '.offset')):
            assert float(g.abs().max()) > 10 * 5e-5 * gmax, n
    (g_loss, _, _), grads = _step(model, model.g_optim, model.g_vars,
                                  lambda: model.g_step(images.to(dev), labels.to(dev)))
    _compare(float(g_loss), grads, ref_loss, ref_grads, names)


def test_a_dropped_label_cannot_pass(dev):
    """On the float64 side alone: with the real batch's labels rolled by one
    the embedding's gradient leaves the true one by more than ten times its
    bound, so a step that lost or misrouted the labels fails the comparison
    above."""
    model, images, labels, z, y = build(dev)
    with torch.no_grad():
        fake = model.generator(z.to(dev), y.to(dev))
    _, ref_grads, names = critic_reference(model, images, labels, y, fake)
    _, bad_grads, _ = critic_reference(model, images, labels.roll(1), y, fake)
    i = names.index('embed.weight')
    tol = tolerances(ref_grads)[0][i]
    excess = (bad_grads[i] - ref_grads[i]).abs().numpy() / tol
    print('embedding gradient: permuted labels differ by up to %.1f x the bound' % excess.max())
    assert excess.max() > 10.0


def test_checkpoint_round_trip(dev, tmp_path):
    a, images, labels, _, _ = build(dev)
    a.sample_y = type(a).sample_y.__get__(a)
    a.sample_z = type(a).sample_z.__get__(a)
    for _ in range(2):
        a.train_step(images.to(dev), labels.to(dev))
    a.save_checkpoint(str(tmp_path), a.step)
    torch.manual_seed(7)
    from gan.core.smmd import SMMD
    b = SMMD(_cfg(), device=dev)
    assert not torch.equal(a.discriminator.embed.weight, b.discriminator.embed.weight)
    assert b.load_checkpoint(str(tmp_path))
    for (na, pa), (nb, pb) in zip(a.generator.state_dict().items(),
                                  b.generator.state_dict().items()):
        assert na == nb and torch.equal(pa, pb), na
    for (na, pa), (nb, pb) in zip(a.discriminator.state_dict().items(),
                                  b.discriminator.state_dict().items()):
        assert na == nb and torch.equal(pa, pb), na
    assert torch.equal(a.d_optim.flat_param, b.d_optim.flat_param)
    assert torch.equal(a.g_optim.m, b.g_optim.m)
    for ea, eb in zip(a.sn_D.entries, b.sn_D.entries):
        assert torch.equal(ea.u, eb.u)
    b.train_step(images.to(dev), labels.to(dev))
    b.check_finite()
