"""GPU parity of the 5x5 stride-2 convolution kernels (csrc/smmd_conv5s2.hip,
`smmd_conv5s2*`): forward, input gradient and weight gradient through convops'
launchers against torch's float64 conv2d / autograd on the host, and the DCGAN
critic through its second-order rule against the same module on MIOpen.
Tolerance 2e-6 of max|ref| (torch's own float32 CPU conv measures 1.0e-7 to
8.3e-7 of max|ref| on these shapes in all three directions).
Measured on an MI355X: forward 3.6e-7 to 5.3e-7, input gradient 2.8e-7 to
5.5e-7, weight gradient 7.8e-8 to 1.6e-7."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 2e-6

# (N, cin, cout, H, W, pad): a partial pixel tile on an image smaller than the
# filter's reach; two cout tiles; non-square with several chunks and a pixel
# tile spanning image rows; symmetric padding (zero taps on all four sides);
# even H (an input row no tap reaches in some phases); the split reduction
SHAPES = [(3, 64, 64, 7, 7, 0), (2, 64, 128, 11, 11, 0), (1, 128, 64, 19, 35, 0),
          (2, 64, 64, 9, 9, 2), (2, 64, 64, 8, 10, 0), (4, 512, 64, 7, 7, 0)]
SPLIT = (4, 512, 64, 7, 7, 0)
_CASES = {}


@pytest.fixture(autouse=True)
def conv5_on():
    """Every supported shape on the library (the default routing keeps the
    shapes on MIOpen that were not measured faster)."""
    from gan.core import convops
    saved = convops.CONV5, convops.CONV5_ALL
    convops.CONV5 = convops.CONV5_ALL = True
    yield
    convops.CONV5, convops.CONV5_ALL = saved


def _case(shape):
    """Seeded inputs and the float64 references of one shape, computed once."""
    if shape not in _CASES:
        N, ci, co, H, W, pad = shape
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(N, ci, H, W, generator=g)
        w = torch.randn(co, ci, 5, 5, generator=g)
        b = torch.randn(co, generator=g)
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y = F.conv2d(xd, wd, b.double(), stride=2, padding=pad)
        gy = torch.randn(y.shape, generator=g)
        gx, gw = torch.autograd.grad(y, (xd, wd), gy.double())
        _CASES[shape] = dict(x=x, w=w, b=b, gy=gy, y=y.detach(), gx=gx, gw=gw)
    return _CASES[shape]


def _rel(a, ref):
    r = ((a.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print('rel err %.3g' % r)
    return r


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_vs_float64(shape):
    from gan.core import _lib, convops
    c = _case(shape)
    x, w, b = (c[k].to(DEV) for k in 'xwb')
    pad = (shape[5], shape[5])
    assert convops._is_k5s2(x, w, (2, 2), pad)
    if shape == SPLIT:
        d = convops._k5s2_dims(x.shape, w.shape[0], pad)
        assert _lib.lib().smmd_conv5s2_workspace_bytes(*d) > 0
    assert _rel(convops._k5s2_conv(x, w, b, pad), c['y']) < TOL


@pytest.mark.parametrize('shape', SHAPES)
def test_input_gradient_vs_float64(shape):
    from gan.core import convops
    c = _case(shape)
    gy, w = c['gy'].to(DEV), c['w'].to(DEV)
    gx = convops._k5s2_dx(gy, w, c['x'].shape, (shape[5], shape[5]))
    assert _rel(gx, c['gx']) < TOL
    # input elements no output reaches are written as exact zeros
    assert torch.equal(gx.cpu()[c['gx'] == 0], torch.zeros(int((c['gx'] == 0).sum())))


@pytest.mark.parametrize('shape', SHAPES)
def test_weight_gradient_vs_float64(shape):
    from gan.core import _lib, convops
    c = _case(shape)
    gy, x = c['gy'].to(DEV), c['x'].to(DEV)
    pad = (shape[5], shape[5])
    if shape == SPLIT:
        d = convops._k5s2_dims(x.shape, gy.shape[1], pad)
        assert _lib.lib().smmd_conv5s2_wgrad_workspace_bytes(*d) > 0
    gw = convops._k5s2_wgrad(gy, x, pad)
    assert _rel(gw, c['gw']) < TOL
    if shape == SHAPES[1]:          # _acc: gw0 + dW
        gw0 = torch.randn(gw.shape, generator=torch.Generator().manual_seed(5))
        acc = convops._k5s2_wgrad(gy, x, pad, into=gw0.to(DEV))
        assert _rel(acc, gw0.double() + c['gw']) < TOL


def _second_order(D, x0, bank):
    if bank is not None:
        bank.refresh(update_u=False)
    x = x0.clone().requires_grad_(True)
    y = D(x)
    gx, = torch.autograd.grad(y.sum(), x, create_graph=True)
    gx.pow(2).sum().backward()
    # (a bias has no second-order gradient: its .grad stays None)
    out = [y.detach(), gx.detach()] + [p.grad.clone() for p in D.parameters()
                                       if p.grad is not None]
    assert len(out) >= 2 + len(D.convs)
    D.zero_grad()
    return out


@pytest.mark.parametrize('with_sn', [False, True])
def test_dcgan_critic_second_order_vs_miopen(with_sn):
    """The critic's forward, input gradient and the double backward of its
    squared norm: the library against MIOpen (the tolerance of the model tests'
    library-versus-MIOpen comparisons), bit-identical run to run, and the
    forward seen on the library's launch record."""
    from gan.core import _lib, convops
    from gan.core.architecture import DCGANDiscriminator
    from gan.core.sn import SpectralNormBank
    from gan.core.snops import sn_modules
    torch.manual_seed(3)
    D = DCGANDiscriminator(dim=64, o_dim=1, use_batch_norm=False, with_sn=with_sn,
                           input_size=16, layers=2).to(DEV)
    x0 = torch.rand(4, 3, 16, 16, device=DEV)
    bank = SpectralNormBank(sn_modules(D)) if with_sn else None
    if bank is not None:
        bank.refresh(update_u=False)
    _lib.reset_timing()
    _lib.enable_timing(True)
    try:
        D(x0)
        assert 'smmd_conv5s2' in _lib.timing_ms()
    finally:
        _lib.enable_timing(False)
        _lib.reset_timing()
    # (the 3-channel first layer stays on MIOpen, whose default weight
    # gradient is not bitwise reproducible: its deterministic mode for it)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        got, again = _second_order(D, x0, bank), _second_order(D, x0, bank)
        convops.CONV5 = False
        ref = _second_order(D, x0, bank)
    finally:
        torch.backends.cudnn.deterministic = det
    for i, (a, a2, r) in enumerate(zip(got, again, ref)):
        print(i, tuple(a.shape), 'rerun diff %.3g' % (a - a2).abs().max().item(),
              'vs MIOpen %.3g of %.3g' % ((a - r).abs().max().item(), r.abs().max().item()))
    for a, a2, r in zip(got, again, ref):
        assert torch.equal(a, a2)
        assert (a - r).abs().max().item() <= 1e-4 * r.abs().max().item() + 1e-7
