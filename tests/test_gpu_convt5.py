"""GPU parity of the wide 5x5 stride-2 transposed conv kernel
(csrc/smmd_conv5s2t.hip, `smmd_conv5s2t`): the launcher and snops.Deconv2d with
its backward on smmd_conv5s2 / smmd_conv5s2_wgrad against torch's float64
transposed conv on the host, cropped to twice the input (bound 2e-6 of
max|ref|, the project's conv bound: torch's own float32 CPU transposed conv
measures at most 8.1e-7 on these seeded inputs; it measured 1.1e-6 at (5, 128,
64, 4, 4) and 1.2e-6 at (2, 512, 64, 2, 2), above 1e-6 on its own, so those two
shapes run at cin = 96 and cin = 384: still several chunks, still split)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 2e-6

# (N, cin, cout, h, w): every tap at a border and a mostly empty pixel tile;
# two channel tiles and a partial tile spanning images; an image straddling two
# pixel tiles and several chunks; odd and non-square; several tiles inside one
# image; the channel split (one tile, 96 chunks)
SHAPES = [(2, 64, 64, 2, 2), (3, 64, 128, 4, 4), (5, 96, 64, 4, 4), (2, 64, 64, 5, 7),
          (1, 64, 64, 16, 16), (2, 384, 64, 2, 2)]
SPLIT = (2, 384, 64, 2, 2)
NO_BIAS = (2, 64, 64, 5, 7)
_CASES = {}


@pytest.fixture(autouse=True)
def convt5_on():
    """Every supported shape and direction on the library, whatever the
    default routing."""
    from gan.core import convops
    saved = convops.CONVT5, convops.CONVT5_ALL, convops.CONV5_ALL
    convops.CONVT5 = convops.CONVT5_ALL = convops.CONV5_ALL = True
    yield
    convops.CONVT5, convops.CONVT5_ALL, convops.CONV5_ALL = saved


def _case(shape):
    """Seeded inputs and the float64 reference of one shape, computed once."""
    if shape not in _CASES:
        N, ci, co, h, w = shape
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn(N, ci, h, w, generator=g)
        wt = torch.randn(ci, co, 5, 5, generator=g)
        b = None if shape == NO_BIAS else torch.randn(co, generator=g)
        y = F.conv_transpose2d(x.double(), wt.double(), None if b is None else b.double(), 2,
                               1)[:, :, :2 * h, :2 * w]
        _CASES[shape] = dict(x=x, w=wt, b=b, y=y)
    return _CASES[shape]


def _rel(a, ref):
    r = ((a.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print('rel err %.3g' % r)
    return r


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_launcher_vs_float64(shape):
    from gan.core import _lib, convops
    c = _case(shape)
    x, w = c['x'].to(DEV), c['w'].to(DEV)
    b = None if c['b'] is None else c['b'].to(DEV)
    assert convops.convt5_applicable(x, w)
    y = convops._convt5(x, w, b)
    assert y.shape == c['y'].shape and _rel(y, c['y']) <= TOL
    if shape == SPLIT:
        assert _lib.lib().smmd_conv5s2t_workspace_bytes(*shape) > 0
        assert torch.equal(y, convops._convt5(x, w, b))


@pytest.mark.parametrize('N,cin,cout,hin', [(2, 64, 64, 4), (2, 128, 64, 3)])
def test_deconv_module_and_gradients(N, cin, cout, hin):
    """snops.Deconv2d(cin, cout) on the device: the forward on smmd_conv5s2t,
    the gradients with respect to x, weight and bias against float64."""
    from gan.core import _lib
    from gan.core.snops import Deconv2d
    torch.manual_seed(N + cin + cout + hin)
    L = Deconv2d(cin, cout)
    with torch.no_grad():
        L.weight.normal_()
        L.bias.normal_()
    x = torch.randn(N, cin, hin, hin)
    gy = torch.randn(N, cout, 2 * hin, 2 * hin)
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
        assert 'smmd_conv5s2t' in _lib.timing_ms()
        got = [y] + list(torch.autograd.grad(y, (xg, L.weight, L.bias), gy.to(DEV)))
        assert {'smmd_conv5s2', 'smmd_conv5s2_wgrad'} <= set(_lib.timing_ms())
    finally:
        _lib.enable_timing(False)
        _lib.reset_timing()
    for a, r in zip(got, ref):
        assert a.shape == r.shape and _rel(a, r) <= TOL
