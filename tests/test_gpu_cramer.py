"""The Cramer head and seed kernels (csrc/smmd_cramer.hip) through the C ABI
against float64 torch autograd on the CPU from the same fp32 inputs.

Bounds, in the form tests/test_gpu_gp.py derives.  Losses: within 1e-5 times
the batch mean of the sum of the norms' magnitudes (the signed norms cancel;
a fixed-order double sum of b <= 70 terms rounded once to fp32 is within
2^-24 of that anchor).  Row gradients, U, gH, gG: |err| <= 1e-5 max|ref| +
1e-5 |ref| per array (each element is formed in double and rounded once, so
the error is the fp32 rounding of the output, 6e-8 |ref|).
"""
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

EPS = 1.0e-5
SHAPES = [(1, 1),
          (3, 5),          # ragged against every vector width
          (5, 64),         # exactly one lane round
          (4, 260),        # float4 plus a partial round
          (3, 1025),       # past the register-resident form, rows off 16 bytes
          (2, 2048),
          (70, 16)]        # five blocks: the partial slab and the ticket


def _n(v):
    return torch.sqrt((v * v).sum(1) + EPS)


def _inputs(b, d):
    gen = torch.Generator().manual_seed(1009 * b + d)
    g, g2, x, h, w = (torch.randn(b, d, generator=gen) for _ in range(5))
    g2[0] = g[0]                   # n(g - g2) = sqrt(eps) and a zero gradient
    x[min(1, b - 1)] = 0.0         # an all-zero real row
    return g, g2, x, h, w


def _reference(variant, g, g2, x, h, w):
    G, G2, X, H = (t.double().requires_grad_(True) for t in (g, g2, x, h))
    if variant == 0:
        terms_g = [-_n(G - G2), _n(G - X), _n(G2 - X)]
        terms_d = [-_n(X - G), _n(X), _n(G2 - G), -_n(G2)]
    else:
        terms_g = [_n(X - G), -_n(X), -_n(G - G2), _n(G)]
        terms_d = [-t for t in terms_g]
    ref = {}
    for key, terms in (('d', terms_d), ('g', terms_g)):
        loss = sum(terms).mean()
        ref[key] = (float(loss.detach()), float(sum(t.abs() for t in terms).mean().detach()),
                    torch.autograd.grad(loss, (G, G2, X), retain_graph=True))
    U, = torch.autograd.grad((_n(H - G) - _n(H)).sum(), H, create_graph=True)
    ref['U'] = U.detach()
    ref['gH'], ref['gG'] = torch.autograd.grad((U * w.double()).sum(), (H, G))
    return ref


def _buf(b, d, dev, dtype=torch.float32):
    return torch.full((b * d + 8,), float('nan'), device=dev, dtype=dtype)      # 8 guard words


def _head(L, ins, variant, want, ws):
    from gan.core import _lib
    g, g2, x = ins
    b, d = g.shape
    out = torch.empty(2, device=g.device)
    grads = [_buf(b, d, g.device) if want & bit else None for bit in (1, 2) for _ in range(3)]
    _lib.check(L.smmd_cramer_head_fwd(_lib.ptr(g), _lib.ptr(g2), _lib.ptr(x), b, d, variant, EPS,
                                      want, _lib.ptr(out), *[_lib.ptr(t) for t in grads],
                                      _lib.ptr(ws), ws.numel(), _lib.stream_handle(g.device)),
               'smmd_cramer_head_fwd')
    return [out] + grads


def _check(name, got, ref, b, d):
    got = got.cpu()
    assert torch.isnan(got[b * d:]).all(), name + ': wrote past the end'
    got = got[:b * d].view(b, d).double()
    assert torch.isfinite(got).all(), name
    bound = 1e-5 * ref.abs().max() + 1e-5 * ref.abs()
    err = (got - ref).abs()
    print('%s: worst err / bound %.3g' % (name, float((err / bound.clamp_min(1e-300)).max())))
    assert (err <= bound).all(), name


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('variant', [0, 1], ids=['cramer', 'reddit_cramer'])
def test_cramer_kernels(dev, variant, shape):
    from gan.core import _lib
    L = _lib.lib()
    b, d = shape
    cpu = _inputs(b, d)
    ref = _reference(variant, *cpu)
    g, g2, x, h, w = (t.to(dev) for t in cpu)
    ws = torch.zeros(L.smmd_cramer_head_workspace_bytes(b, d), dtype=torch.uint8, device=dev)
    both = _head(L, (g, g2, x), variant, 3, ws)
    # a second forward on the same workspace (left at rest), then each mask alone
    for want, keep in ((3, range(1, 7)), (1, (1, 2, 3)), (2, (4, 5, 6))):
        part = _head(L, (g, g2, x), variant, want, ws)
        assert torch.equal(part[0], both[0])
        assert all(torch.equal(part[k][:b * d], both[k][:b * d]) for k in keep)
    out = both[0].cpu().double()
    for k, key in enumerate('dg'):
        loss, anchor, grads = ref[key]
        print('%s loss: err / bound %.3g' % (key, abs(float(out[k]) - loss) / (1e-5 * anchor)))
        assert abs(float(out[k]) - loss) <= 1e-5 * anchor
        for j, name in enumerate(('G', 'G2', 'X')):
            _check('d %s / d %s' % (key, name), both[1 + 3 * k + j], grads[j], b, d)
    # the seed and its backward
    U, gH, gG = (_buf(b, d, dev) for _ in range(3))
    norms = torch.empty(b, 2, device=dev, dtype=torch.float64)
    s = _lib.stream_handle(dev)
    _lib.check(L.smmd_cramer_seed_fwd(_lib.ptr(h), _lib.ptr(g), b, d, EPS, _lib.ptr(U),
                                      _lib.ptr(norms), s), 'smmd_cramer_seed_fwd')
    _lib.check(L.smmd_cramer_seed_bwd(_lib.ptr(h), _lib.ptr(g), _lib.ptr(norms), _lib.ptr(w), b, d,
                                      _lib.ptr(gH), _lib.ptr(gG), s), 'smmd_cramer_seed_bwd')
    for name, got in (('U', U), ('gH', gH), ('gG', gG)):
        _check(name, got, ref[name], b, d)
    ref_n = torch.stack([_n(cpu[3].double() - cpu[0].double()), _n(cpu[3].double())], 1)
    assert torch.allclose(norms.cpu(), ref_n, rtol=1e-7, atol=0)      # eps is passed in fp32

