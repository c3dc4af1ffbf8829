"""The gradient-penalty and critic-head kernels (csrc/smmd_gp.hip) on the GPU
against float64 evaluated here from the same fp32 inputs.

Bounds.  Penalty: rtol 1e-5 -- a fixed-order sum of n <= 2^15 non-negative
terms, each a few ulp off, is within about (log2 n + 6) 2^-24 = 1.3e-6.  dg:
|dg - ref| <= 1e-5 max|ref| + 1e-5 |ref| -- (s - 1) cancels near s = 1 with an
absolute error of about 4 * 2^-24 s, so the bound is anchored to the tensor's
maximum.  Slopes (eps = 0): rtol 2e-6.  Interpolates: bit-equal to the same
expression in separate torch fp32 ops (the kernel contracts nothing).  Head:
losses rtol 1e-5 / atol 1e-7, row gradients rtol 1e-5 / atol 1e-9.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 4, 4),        # fewer pixels than one wave
          (3, 3, 5, 7),        # ragged against every vector width and block size
          (4, 1, 8, 8),        # c = 1
          (8, 3, 64, 64)]      # 32 blocks: the second reduction level


def _grad(shape, cl, dev, seed=0):
    """Gaussian g scaled per sample so the slopes spread over ~0.1 .. 3."""
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen)
    scale = torch.logspace(-1, 0.5, b).view(b, 1, 1, 1) / (c ** 0.5)
    g = (g * scale).to(dev)
    if cl:
        g = g.contiguous(memory_format=torch.channels_last)
    return g


def _slope_ref(g, eps=0.0):
    g64 = g.detach().double().cpu()
    s = torch.sqrt((g64 * g64).sum(1) + eps)              # [b, h, w]
    n = s.numel()
    pen = ((s - 1.0) ** 2).mean()
    dg = (2.0 * (s - 1.0) / (s * n)).unsqueeze(1) * g64
    return s.reshape(-1), pen, dg


def _raw_slope(g, cl, eps, go=1.0):
    """(out, slopes, dg) straight from the C ABI."""
    from gan.core import _lib
    L = _lib.lib()
    b, c, h, w = g.shape
    dev = g.device
    out = torch.empty(1, device=dev)
    slopes = torch.empty(b * h * w, device=dev)
    nb = L.smmd_gp_slope_workspace_bytes(b, c, h * w)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    s = _lib.stream_handle(dev)
    _lib.check(L.smmd_gp_slope_fwd(_lib.ptr(g), b, c, h * w, int(cl), eps, _lib.ptr(out),
                                   _lib.ptr(slopes), _lib.ptr(ws), nb, s), 'slope_fwd')
    got = torch.tensor([go], device=dev)
    dg = torch.empty_like(g)
    assert dg.stride() == g.stride()
    _lib.check(L.smmd_gp_slope_bwd(_lib.ptr(g), _lib.ptr(slopes), b, c, h * w, int(cl),
                                   _lib.ptr(got), _lib.ptr(dg), s), 'slope_bwd')
    # a second forward on the same workspace: the ticket was left at rest
    out2 = torch.empty(1, device=dev)
    _lib.check(L.smmd_gp_slope_fwd(_lib.ptr(g), b, c, h * w, int(cl), eps, _lib.ptr(out2),
                                   _lib.ptr(slopes), _lib.ptr(ws), nb, s), 'slope_fwd')
    assert torch.equal(out, out2)
    return out, slopes, dg


@pytest.mark.parametrize('cl', [False, True], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('eps', [0.0, 1e-8])
def test_slope_kernels(dev, shape, cl, eps):
    g = _grad(shape, cl, dev)
    s_ref, pen_ref, dg_ref = _slope_ref(g, eps)
    assert (s_ref < 0.5).any() and (s_ref > 1.5).any()
    out, slopes, dg = _raw_slope(g, cl, eps, go=0.75)
    pen, s = float(out.cpu()), slopes.cpu().double()
    print('penalty rel err %.3g' % (abs(pen - float(pen_ref)) / float(pen_ref)))
    assert pen == pytest.approx(float(pen_ref), rel=1e-5)
    print('slopes max rel err %.3g' % float(((s - s_ref).abs() / s_ref).max()))
    assert torch.allclose(s, s_ref, rtol=2e-6, atol=0)
    ref = 0.75 * dg_ref
    got = dg.cpu().double()                         # logical NCHW values either way
    err = (got - ref).abs()
    bound = 1e-5 * ref.abs().max() + 1e-5 * ref.abs()
    print('dg max err / bound %.3g' % float((err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('b', [2, 3])
@pytest.mark.parametrize('per', [3 * 4 * 4, 3 * 5 * 7, 3 * 64 * 64])
def test_interp_bit_equal(dev, per, b, form):
    """Bit-equal to the expression in separate torch fp32 ops, in the stated
    order: the kernel rounds every operation on its own (no contraction)."""
    from gan.core import _lib
    gen = torch.Generator().manual_seed(per + b)
    real = torch.randn(b, per, generator=gen).to(dev)
    fake = torch.randn(b, per, generator=gen).to(dev)
    alpha = torch.rand(b, 1, generator=gen).to(dev)
    out = torch.full((b * per + 8,), float('nan'), device=dev)      # 8 guard words
    st = _lib.lib().smmd_gp_interp(_lib.ptr(real), _lib.ptr(fake), _lib.ptr(alpha),
                                   _lib.ptr(out), b, per, form, _lib.stream_handle(dev))
    _lib.check(st, 'smmd_gp_interp')
    if form == 0:
        ref = real + alpha * (fake - real)
    else:
        ref = (1.0 - alpha) * real + alpha * fake
    assert torch.equal(out[:b * per].view(b, per), ref)
    assert torch.isnan(out[b * per:]).all()                        # nothing past the end


def test_interp_op_formats_and_offsets(dev):
    """ops.gp_interpolate: memory formats kept, and a base off 16 bytes (a
    view with a storage offset) takes the element-wise path."""
    from gan.core import _lib, ops
    gen = torch.Generator().manual_seed(5)
    real = torch.randn(3, 3, 5, 7, generator=gen).to(dev)
    fake = torch.randn(3, 3, 5, 7, generator=gen).to(dev)
    alpha = torch.rand(3, 1, 1, 1, generator=gen).to(dev)
    ref = real + alpha * (fake - real)
    out = ops.gp_interpolate(real, fake, alpha, 0)
    assert out.is_contiguous() and torch.equal(out, ref) and not out.requires_grad
    rc = real.contiguous(memory_format=torch.channels_last)
    out = ops.gp_interpolate(rc, fake, alpha, 0)
    assert out.is_contiguous(memory_format=torch.channels_last) and torch.equal(out, ref)
    buf_r = torch.zeros(3 * 105 + 1, device=dev)
    buf_f = torch.zeros(3 * 105 + 1, device=dev)
    buf_r[1:] = real.reshape(-1)
    buf_f[1:] = fake.reshape(-1)
    r1, f1 = buf_r[1:].view(3, 105), buf_f[1:].view(3, 105)
    assert r1.data_ptr() % 16 == 4
    out = torch.empty(3, 105, device=dev)
    st = _lib.lib().smmd_gp_interp(_lib.ptr(r1), _lib.ptr(f1), _lib.ptr(alpha), _lib.ptr(out),
                                   3, 105, 0, _lib.stream_handle(dev))
    _lib.check(st, 'smmd_gp_interp')
    assert torch.equal(out.view(3, 3, 5, 7), ref)


def _head_inputs(n, kind, dev):
    gen = torch.Generator().manual_seed(n)
    xr = torch.randn(n, 1, generator=gen) * 2.0
    xf = torch.randn(n, 1, generator=gen) * 2.0 + 0.5
    if kind == 1:                      # stable softplus: the far tails, both signs
        if n >= 4:
            xr[:4, 0] = torch.tensor([30.0, -30.0, 100.0, -100.0])
            xf[:4, 0] = torch.tensor([-100.0, 100.0, -30.0, 30.0])
        else:
            xr[:2, 0] = torch.tensor([100.0, -30.0])
            xf[:2, 0] = torch.tensor([30.0, -100.0])
    return xr.to(dev), xf.to(dev)


def _softplus64(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def _head_ref(xr, xf, kind):
    r = xr.detach().double().cpu().requires_grad_(True)
    f = xf.detach().double().cpu().requires_grad_(True)
    if kind == 0:
        o0, o1 = f.mean() - r.mean(), -f.mean()
    else:
        o0 = _softplus64(-r).mean() + _softplus64(f).mean()
        o1 = _softplus64(-f).mean()
    g_real, g_fake = torch.autograd.grad(o0, (r, f), retain_graph=True)
    gg_fake, = torch.autograd.grad(o1, f)
    return o0.detach(), o1.detach(), g_real, g_fake, gg_fake


def _raw_head(xr, xf, kind):
    from gan.core import _lib
    dev = xr.device
    out = torch.empty(2, device=dev)
    g_real, g_fake, gg_fake = torch.empty_like(xr), torch.empty_like(xf), torch.empty_like(xf)
    st = _lib.lib().smmd_critic_head_fwd(_lib.ptr(xr), xr.numel(), _lib.ptr(xf), xf.numel(), kind,
                                         _lib.ptr(out), _lib.ptr(g_real), _lib.ptr(g_fake),
                                         _lib.ptr(gg_fake), _lib.stream_handle(dev))
    _lib.check(st, 'smmd_critic_head_fwd')
    return out, g_real, g_fake, gg_fake


@pytest.mark.parametrize('kind', [0, 1], ids=['wgan', 'gan'])
@pytest.mark.parametrize('n', [2, 6, 64, 256])
def test_head_kernel(dev, n, kind):
    xr, xf = _head_inputs(n, kind, dev)
    o0, o1, g_real, g_fake, gg_fake = _head_ref(xr, xf, kind)
    out, gr, gf, ggf = _raw_head(xr, xf, kind)
    assert torch.isfinite(out).all()
    np.testing.assert_allclose(out.cpu().double().numpy(), [float(o0), float(o1)],
                               rtol=1e-5, atol=1e-7)
    for got, ref in ((gr, g_real), (gf, g_fake), (ggf, gg_fake)):
        assert torch.isfinite(got).all()
        np.testing.assert_allclose(got.cpu().double().numpy(), ref.numpy(), rtol=1e-5, atol=1e-9)


def test_head_softplus_of_100_is_100(dev):
    xr = torch.tensor([[-100.0]], device=dev)          # softplus(-real) = softplus(100)
    xf = torch.tensor([[100.0]], device=dev)
    out, gr, gf, ggf = _raw_head(xr, xf, 1)
    assert float(out[0]) == 200.0 and 0.0 <= float(out[1]) < 1e-40
    assert float(gr) == -1.0 and float(gf) == 1.0


def test_two_runs_same_bits(dev):
    for cl in (False, True):
        g = _grad((8, 3, 64, 64), cl, dev, seed=7)
        a = _raw_slope(g, cl, 0.0)
        b = _raw_slope(g, cl, 0.0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for kind in (0, 1):
        xr, xf = _head_inputs(256, kind, dev)
        a, b = _raw_head(xr, xf, kind), _raw_head(xr, xf, kind)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('cl', [False, True], ids=['nchw', 'nhwc'])
def test_slope_penalty_autograd(dev, cl):
    from gan.core import ops
    g = _grad((3, 3, 5, 7), cl, dev).requires_grad_(True)
    p = ops.slope_penalty(g, 0.0)
    assert p.dim() == 0
    (3.0 * p).backward()
    _, _, dg = _raw_slope(g.detach(), cl, 0.0, go=3.0)
    assert g.grad.stride() == g.stride() and torch.equal(g.grad, dg)
    _, pen_ref, dg_ref = _slope_ref(g)
    assert float(p.detach()) == pytest.approx(float(pen_ref), rel=1e-5)
    err = (g.grad.cpu().double() - 3.0 * dg_ref).abs()
    assert (err <= 3e-5 * dg_ref.abs().max() + 1e-5 * 3.0 * dg_ref.abs()).all()


@pytest.mark.parametrize('kind', [0, 1], ids=['wgan', 'gan'])
def test_critic_head_loss_autograd(dev, kind):
    from gan.core import ops
    xr, xf = _head_inputs(6, kind, dev)
    xr.requires_grad_(True)
    xf.requires_grad_(True)
    d_base, g_loss = ops.critic_head_loss(xr, xf, kind)
    assert d_base.dim() == 0 and g_loss.dim() == 0
    gr, gf = torch.autograd.grad(2.0 * d_base + 0.5 * g_loss, (xr, xf))
    o0, o1, g_real, g_fake, gg_fake = _head_ref(xr, xf, kind)
    assert float(d_base.detach()) == pytest.approx(float(o0), rel=1e-5, abs=1e-7)
    assert float(g_loss.detach()) == pytest.approx(float(o1), rel=1e-5, abs=1e-7)
    assert gr.shape == xr.shape and gf.shape == xf.shape
    np.testing.assert_allclose(gr.cpu().double().numpy(), (2.0 * g_real).numpy(),
                               rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(gf.cpu().double().numpy(), (2.0 * g_fake + 0.5 * gg_fake).numpy(),
                               rtol=2e-5, atol=1e-9)


def test_fused_switch_off_matches(dev, monkeypatch):
    """SMMD_GP_FUSED=0's plain-tensor path computes the same things."""
    from gan.core import ops
    g = _grad((3, 3, 5, 7), False, dev)
    fused = ops.slope_penalty(g, 0.0)
    monkeypatch.setattr(ops, 'GP_FUSED', False)
    plain = ops.slope_penalty(g, 0.0)
    assert float(fused) == pytest.approx(float(plain), rel=1e-5)
