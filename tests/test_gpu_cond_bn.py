"""Conditional batch norm + ReLU on the GPU (csrc/smmd_cond_bn.hip through
snops.cond_bn_relu) against the formula in float64 written here
(resnet/ops/cond_batchnorm.py:6-17 then tf.nn.relu, resnet/block.py:42-47).

Bounds are those of the unconditional kernel's tests
(tests/test_gpu_relupool.py::test_bn_relu_backward_matches_float64): output
|d| <= 2e-5 max|ref| + 1e-6, gradients |d| <= 1e-4 max|ref| + 1e-6."""
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

# (N, C, H, W, K), how the labels are drawn
SHAPES = [((2, 3, 2, 2, 2), 'random'),          # smallest, HW = 4
          ((5, 7, 4, 4, 3), 'random'),          # odd N and C
          ((8, 64, 8, 8, 5), 'one'),            # one class: the other rows exactly 0
          ((6, 16, 4, 4, 6), 'each'),           # one sample per class
          ((3, 8, 16, 16, 1000), 'random'),     # table far larger than the batch
          ((4, 5, 2, 3, 3), 'random')]          # HW = 6: the torch path


def _case(shape, labels, dev, seed_add=0):
    N, C, H, W, K = shape
    g = torch.Generator().manual_seed(sum(shape) + seed_add)
    x = torch.randn(N, C, H, W, generator=g) * 3 + 1
    gy = torch.randn(N, C, H, W, generator=g)
    gy = torch.where(gy >= 0, gy + 0.5, gy - 0.5)        # |gy| >= 0.5: a mask shows in gx
    scale = torch.rand(K, C, generator=g) + 0.5
    offset = torch.randn(K, C, generator=g)
    if labels == 'one':
        y = torch.full((N,), 3)
    elif labels == 'each':
        y = torch.randperm(N, generator=g)
    else:
        y = torch.randint(0, K, (N,), generator=g)
    return [t.to(dev) for t in (x, gy, scale, offset, y)]


def _ref64(x, gy, scale, offset, y, eps=1e-5):
    """(y, z, gx, gscale, goffset, parts) in float64 by autograd on the formula."""
    x = x.double().requires_grad_(True)
    s = scale.double().requires_grad_(True)
    o = offset.double().requires_grad_(True)
    mean = x.mean((0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((0, 2, 3), keepdim=True)
    inv = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * inv
    z = xh * s[y][:, :, None, None] + o[y][:, :, None, None]
    out = torch.relu(z)
    out.backward(gy.double())
    return out.detach(), z.detach(), x.grad, s.grad, o.grad, (inv.detach(), xh.detach())


def _run(x, gy, scale, offset, y):
    from gan.core.snops import CondBatchNorm2d, cond_bn_relu
    bn = CondBatchNorm2d(scale.shape[0], scale.shape[1]).to(x.device)
    with torch.no_grad():
        bn.scale.copy_(scale)
        bn.offset.copy_(offset)
    xx = x.clone().requires_grad_(True)
    out = cond_bn_relu(bn, xx, y)
    out.backward(gy)
    return out.detach(), xx.grad, bn.scale.grad, bn.offset.grad, type(out.grad_fn).__name__


def _close(got, ref, rel):
    err = float((got.double() - ref).abs().max())
    assert err <= rel * float(ref.abs().max()) + 1e-6, (err, float(ref.abs().max()))


@pytest.mark.parametrize('shape,labels', SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_cond_bn_relu_matches_float64(dev, monkeypatch, shape, labels):
    from gan.core import snops
    monkeypatch.setattr(snops, 'COND_BN', True)
    x, gy, scale, offset, y = _case(shape, labels, dev)
    ref_y, _, ref_gx, ref_gs, ref_go, _ = _ref64(x, gy, scale, offset, y)
    out, gx, gs, go, node = _run(x, gy, scale, offset, y)
    fused = (shape[2] * shape[3]) % 4 == 0
    assert ('CondBNReLU' in node) == fused               # HW = 6 takes the torch ops
    _close(out, ref_y, 2e-5)
    for got, ref in ((gx, ref_gx), (gs, ref_gs), (go, ref_go)):
        _close(got, ref, 1e-4)
    # without a gradient: the same forward, no record kept
    from gan.core.snops import CondBatchNorm2d, cond_bn_relu
    bn = CondBatchNorm2d(shape[4], shape[1]).to(dev)
    with torch.no_grad():
        bn.scale.copy_(scale)
        bn.offset.copy_(offset)
        assert torch.equal(cond_bn_relu(bn, x, y), out)
        # int32 labels (what the generator hands every layer) read the same rows
        assert torch.equal(cond_bn_relu(bn, x, y.to(torch.int32)), out)


def test_absent_classes_get_exact_zeros(dev, monkeypatch):
    """Every row of both tables' gradients is written: with all samples in
    class 3 the other rows are exactly 0, whatever the memory held."""
    from gan.core import _lib, snops
    monkeypatch.setattr(snops, 'COND_BN', True)
    shape, labels = SHAPES[2]
    N, C, H, W, K = shape
    x, gy, scale, offset, y = _case(shape, labels, dev)
    L = _lib.lib()
    y32 = y.to(torch.int32)
    ws = torch.zeros(L.smmd_cond_bn_relu_workspace_bytes(N, C), dtype=torch.uint8, device=dev)
    out, save = torch.empty_like(x), torch.empty(3 * C, device=dev)
    st = L.smmd_cond_bn_relu_fwd(_lib.ptr(x), _lib.ptr(y32), N, C, H * W, K, _lib.ptr(scale),
                                 _lib.ptr(offset), 1e-5, _lib.ptr(out), _lib.ptr(save),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
    assert st == 0
    nan = float('nan')
    gx = torch.full_like(x, nan)
    gs, go = torch.full_like(scale, nan), torch.full_like(offset, nan)
    st = L.smmd_cond_bn_relu_bwd(_lib.ptr(x), _lib.ptr(gy), _lib.ptr(y32), N, C, H * W, K,
                                 _lib.ptr(scale), _lib.ptr(offset), _lib.ptr(save), _lib.ptr(gx),
                                 _lib.ptr(gs), _lib.ptr(go), _lib.ptr(ws), ws.numel(),
                                 _lib.stream_handle(dev))
    assert st == 0
    torch.cuda.synchronize()
    absent = [k for k in range(K) if k != 3]
    assert torch.equal(gs[absent], torch.zeros(K - 1, C, device=dev))
    assert torch.equal(go[absent], torch.zeros(K - 1, C, device=dev))
    _, _, ref_gx, ref_gs, ref_go, _ = _ref64(x, gy, scale, offset, y)
    for got, ref in ((gx, ref_gx), (gs, ref_gs), (go, ref_go)):
        _close(got, ref, 1e-4)


def test_out_of_range_label_is_clamped(dev):
    """The library never reads outside the tables: a label past either end
    reads the nearest row (the Python side refuses such labels earlier)."""
    from gan.core import _lib
    N, C, H, W, K = 4, 8, 4, 4, 3
    x, gy, scale, offset, _ = _case((N, C, H, W, K), 'random', dev)
    L = _lib.lib()
    ws = torch.zeros(L.smmd_cond_bn_relu_workspace_bytes(N, C), dtype=torch.uint8, device=dev)
    outs = []
    for y in ([-7, 0, 2, 1 << 30], [0, 0, 2, 2]):
        y32 = torch.tensor(y, dtype=torch.int32, device=dev)
        out = torch.empty_like(x)
        st = L.smmd_cond_bn_relu_fwd(_lib.ptr(x), _lib.ptr(y32), N, C, H * W, K, _lib.ptr(scale),
                                     _lib.ptr(offset), 1e-5, _lib.ptr(out), None, _lib.ptr(ws),
                                     ws.numel(), _lib.stream_handle(dev))
        assert st == 0
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_relu_mask_is_the_forwards(dev, monkeypatch):
    """(y > 0) is the mask the backward used.  gx = inv (gamma gz - S1 / M -
    xhat S2 / M), so gamma gz = gx / inv + S1 / M + xhat S2 / M is ~0 where
    the backward masked and gamma gy (at least 0.25 in size here) where it did
    not; x is built so that no |z| is under 1e-3 in float64."""
    from gan.core import snops
    monkeypatch.setattr(snops, 'COND_BN', True)
    shape = (5, 7, 4, 4, 3)
    x, gy, scale, offset, y = _case(shape, 'random', dev, seed_add=1)
    _, z, _, _, _, _ = _ref64(x, gy, scale, offset, y)
    near = z.abs() < 1e-2
    x = torch.where(near.to(dev), x + 0.5, x)            # move the few borderline elements
    ref_y, z, ref_gx, ref_gs, ref_go, (inv, xh) = _ref64(x, gy, scale, offset, y)
    assert float(z.abs().min()) > 1e-3
    out, gx, _, _, _ = _run(x, gy, scale, offset, y)
    M = float(shape[0] * shape[2] * shape[3])
    gm = scale.double()[y][:, :, None, None]
    gz = gy.double() * (z > 0)
    s1 = (gm * gz).sum((0, 2, 3), keepdim=True)
    s2 = (gm * gz * xh).sum((0, 2, 3), keepdim=True)
    implied = gx.double() / inv + s1 / M + xh * s2 / M                 # gamma gz
    floor = float((gm * gy.double()).abs().min())
    assert floor >= 0.25
    assert torch.equal(implied.abs() > 0.5 * floor, out > 0)
    assert torch.equal(out > 0, z > 0)


def test_two_runs_give_the_same_bits(dev, monkeypatch):
    from gan.core import snops
    monkeypatch.setattr(snops, 'COND_BN', True)
    for shape, labels in (SHAPES[2], SHAPES[4]):
        case = _case(shape, labels, dev)
        a, b = _run(*case), _run(*case)
        for p, q in zip(a[:4], b[:4]):
            assert torch.equal(p, q)


def test_switch_off_agrees(dev, monkeypatch):
    """SMMD_COND_BN=0 (torch ops in the same arithmetic) within the bounds of
    the fused path, against the same float64 values."""
    from gan.core import snops
    shape, labels = SHAPES[1]
    case = _case(shape, labels, dev)
    ref_y, _, ref_gx, ref_gs, ref_go, _ = _ref64(*case)
    monkeypatch.setattr(snops, 'COND_BN', False)
    out, gx, gs, go, node = _run(*case)
    assert 'CondBNReLU' not in node
    _close(out, ref_y, 2e-5)
    for got, ref in ((gx, ref_gx), (gs, ref_gs), (go, ref_go)):
        _close(got, ref, 1e-4)


def test_double_backward_is_differentiable(dev, monkeypatch):
    """create_graph through _CondBNReLU: the second-order gradient equals the
    torch composition's."""
    from gan.core import snops
    from gan.core.snops import CondBatchNorm2d, cond_bn_relu
    shape = (6, 5, 4, 4, 3)
    x, _, scale, offset, y = _case(shape, 'random', dev)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(snops, 'COND_BN', on)
        bn = CondBatchNorm2d(3, 5).to(dev)
        with torch.no_grad():
            bn.scale.copy_(scale)
            bn.offset.copy_(offset)
        xx = x.clone().requires_grad_(True)
        out = cond_bn_relu(bn, xx, y)
        gx, = torch.autograd.grad((out * out.detach().cos()).sum(), xx, create_graph=True)
        gw, = torch.autograd.grad((gx * gx).sum(), bn.scale)
        outs.append((gx.detach(), gw))
    for a, b in zip(*outs):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))
