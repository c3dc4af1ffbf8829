"""GPU parity of the thin 5x5 stride-2 kernels (csrc/smmd_conv5s2_thin.hip,
`smmd_conv5s2_thin*`): the three directions through convops' launchers and
snops.Deconv2d's TF-SAME transposed geometry against torch's float64 conv on
the host (bound 2e-6 of max|ref|, the project's conv bound: torch's own
float32 CPU conv measures at most 9.9e-7 on these shapes), and the DCGAN
critic through its second-order rule against the same module on MIOpen."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 2e-6

# (N, ct, cw, H, W, pad): an image smaller than one tile; zero taps on all four
# sides and two 32-row cw tiles; non-square with several row bands, a partial
# last band and pixel tiles spanning rows; ct = 1; ct = 4; an even size (a row
# and a column no tap reaches); several slab partials of the weight gradient
SHAPES = [(3, 3, 16, 7, 7, 0), (2, 3, 64, 9, 9, 2), (1, 3, 32, 35, 67, 0), (2, 1, 16, 11, 11, 0),
          (2, 4, 16, 11, 11, 0), (2, 3, 16, 8, 10, 0), (8, 3, 16, 35, 35, 0)]
SLABS = (8, 3, 16, 35, 35, 0)
_CASES = {}


@pytest.fixture(autouse=True)
def thin5_on():
    """Every supported shape on the library, whatever the default routing."""
    from gan.core import convops
    saved = convops.THIN5, convops.THIN5_ALL
    convops.THIN5 = convops.THIN5_ALL = True
    yield
    convops.THIN5, convops.THIN5_ALL = saved


def _case(shape):
    """Seeded inputs and the float64 references of one shape, computed once."""
    if shape not in _CASES:
        N, ct, cw, H, W, pad = shape
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(N, ct, H, W, generator=g)
        w = torch.randn(cw, ct, 5, 5, generator=g)
        b = torch.randn(cw, generator=g)
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
def test_three_directions_vs_float64(shape):
    from gan.core import _lib, convops
    c = _case(shape)
    x, w, b, gy = (c[k].to(DEV) for k in ('x', 'w', 'b', 'gy'))
    pad = (shape[5], shape[5])
    for direction in ('fwd', 'dx', 'wgrad'):
        assert convops._is_thin5(x, w, (2, 2), pad, direction)
    d = convops._thin5_dims(x.shape, w, pad)
    assert _rel(convops._thin5_conv(x, w, b, d), c['y']) <= TOL
    gx = convops._thin5_convt(gy, w, None, d)
    assert _rel(gx, c['gx']) <= TOL
    # thin-side pixels no tap reaches are written as exact zeros
    assert torch.equal(gx.cpu()[c['gx'] == 0], torch.zeros(int((c['gx'] == 0).sum())))
    if shape == (2, 3, 16, 8, 10, 0):
        assert (c['gx'][:, :, 7] == 0).all() and (c['gx'][:, :, :, 9] == 0).all()
    assert _rel(convops._thin5_wgrad(gy, x, d), c['gw']) <= TOL
    if shape == SLABS:
        assert _lib.lib().smmd_conv5s2_thin_wgrad_workspace_bytes(*d) > 0
        gw0 = torch.randn(c['gw'].shape, generator=torch.Generator().manual_seed(5))
        acc = convops._thin5_wgrad(gy, x, d, into=gw0.to(DEV))
        assert _rel(acc, gw0.double() + c['gw']) <= TOL


@pytest.mark.parametrize('N,cw,hin', [(2, 16, 4), (2, 64, 5)])
def test_deconv_tf_same_geometry(N, cw, hin):
    """snops.Deconv2d(cw, 3, 5, 2): output = twice the input, one zero row
    before and two after, against conv_transpose2d(x, w, b, 2, 1) cropped."""
    from gan.core import _lib
    from gan.core.snops import Deconv2d
    torch.manual_seed(N + cw + hin)
    L = Deconv2d(cw, 3, 5, 2)
    with torch.no_grad():
        L.weight.normal_()
        L.bias.normal_()
    x = torch.randn(N, cw, hin, hin)
    gy = torch.randn(N, 3, 2 * hin, 2 * hin)
    xd = x.double().requires_grad_(True)
    wd, bd = L.weight.detach().double().requires_grad_(True), L.bias.detach().double().requires_grad_(True)
    yd = F.conv_transpose2d(xd, wd, bd, 2, 1)[:, :, :2 * hin, :2 * hin]
    ref = [yd.detach()] + list(torch.autograd.grad(yd, (xd, wd, bd), gy.double()))
    L = L.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    _lib.reset_timing()
    _lib.enable_timing(True)
    try:
        y = L(xg)
        assert 'smmd_conv5s2_thin_t' in _lib.timing_ms()
    finally:
        _lib.enable_timing(False)
        _lib.reset_timing()
    got = [y] + list(torch.autograd.grad(y, (xg, L.weight, L.bias), gy.to(DEV)))
    for a, r in zip(got, ref):
        assert a.shape == r.shape and _rel(a, r) <= TOL


@pytest.mark.parametrize('with_sn', [False, True])
def test_dcgan_critic_second_order_vs_miopen(with_sn):
    """The width-16 critic's forward, input gradient and the double backward of
    its squared norm: the library against MIOpen in deterministic mode,
    bit-identical run to run, the first layer seen on the launch record."""
    from gan.core import _lib, convops
    from gan.core.architecture import DCGANDiscriminator
    from gan.core.sn import SpectralNormBank
    from gan.core.snops import sn_modules
    torch.manual_seed(3)
    D = DCGANDiscriminator(dim=16, o_dim=1, use_batch_norm=False, with_sn=with_sn,
                           input_size=16, layers=2).to(DEV)
    x0 = torch.rand(4, 3, 16, 16, device=DEV)
    bank = SpectralNormBank(sn_modules(D)) if with_sn else None

    def second_order():
        if bank is not None:
            bank.refresh(update_u=False)
        x = x0.clone().requires_grad_(True)
        y = D(x)
        gx, = torch.autograd.grad(y.sum(), x, create_graph=True)
        gx.pow(2).sum().backward()
        out = [y.detach(), gx.detach()] + [p.grad.clone() for p in D.parameters()
                                           if p.grad is not None]
        assert len(out) >= 2 + len(D.convs)
        D.zero_grad()
        return out

    if bank is not None:
        bank.refresh(update_u=False)
    _lib.reset_timing()
    _lib.enable_timing(True)
    try:
        D(x0)
        assert 'smmd_conv5s2_thin' in _lib.timing_ms()
    finally:
        _lib.enable_timing(False)
        _lib.reset_timing()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        got, again = second_order(), second_order()
        convops.THIN5 = False
        ref = second_order()
    finally:
        torch.backends.cudnn.deterministic = det
    for i, (a, a2, r) in enumerate(zip(got, again, ref)):
        print(i, tuple(a.shape), 'rerun diff %.3g' % (a - a2).abs().max().item(),
              'vs MIOpen %.3g of %.3g' % ((a - r).abs().max().item(), r.abs().max().item()))
    for a, a2, r in zip(got, again, ref):
        assert torch.equal(a, a2)
        assert (a - r).abs().max().item() <= 1e-4 * r.abs().max().item() + 1e-7
