"""The Sobolev head and weight-decay kernels (csrc/smmd_sobolev.hip) through
the C ABI against float64 evaluated here from the same fp32 inputs.

Bounds, from tests/test_gpu_gp.py's (log2 n + 6) 2^-24 for a fixed-order sum of
non-negative terms.  e_r, e_f: rtol 1e-5.  c = (e_r + e_f) / 2 - 1 cancels, so
|dc| <= cb = 1e-5 (e_r + e_f) / 2, anchored to the sum.  mult = lam + rho c:
rho cb + 1e-6 |ref|.  out[0], whose derivative in c is mult: |mult| cb + rho
cb^2 / 2 + 1e-6 |ref|.  out[1]: rtol 1e-5 / atol 1e-7 as for the existing head.
dg: 2e-5 |ref|.  dd: rtol 1e-6.  Decay: value rtol 1e-5, gradient rtol 1e-6,
exactly 0 outside the segments.
"""
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 3, 4, 4),       # less than a wave
          (3, 2, 3, 5, 7),       # ragged against every vector width, unequal batches
          (4, 4, 1, 8, 8),
          (8, 8, 3, 64, 64)]     # 48 blocks: the second reduction level
GO = 0.75


def _grad(b, chw, target, cl, dev, seed):
    """Gaussian g scaled per sample (as tests/test_gpu_gp.py's _grad) so that
    sum(g^2) / b is about ``target``."""
    per = chw[0] * chw[1] * chw[2]
    g = torch.randn((b,) + chw, generator=torch.Generator().manual_seed(seed))
    w = torch.logspace(-0.5, 0.5, b)
    g = (g * torch.sqrt(target * w / w.mean() / per).view(b, 1, 1, 1)).to(dev)
    return g.contiguous(memory_format=torch.channels_last) if cl else g


@pytest.mark.parametrize('lam,rho', [(0.0, 10.0), (0.37, 10.0), (-0.5, 0.0)])
@pytest.mark.parametrize('cl', [False, True], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_head_kernels(dev, shape, cl, lam, rho):
    from gan.core import _lib
    L = _lib.lib()
    br, bf, chw = shape[0], shape[1], tuple(shape[2:])
    per = chw[0] * chw[1] * chw[2]
    # e_r about 1.6 and e_f about 0.9: c about +0.25, the sign of every lam >= 0
    gr, gf = _grad(br, chw, 1.6, cl, dev, 1), _grad(bf, chw, 0.9, cl, dev, 2)
    gen = torch.Generator().manual_seed(3)
    dr, df = torch.randn(br, generator=gen).to(dev), torch.randn(bf, generator=gen).to(dev)
    lam_t, lam64 = torch.tensor([lam], device=dev), float(torch.tensor(lam).double())
    gr64, gf64, dr64, df64 = (t.double().cpu() for t in (gr, gf, dr, df))
    er, ef = float((gr64 * gr64).sum() / br), float((gf64 * gf64).sum() / bf)
    c = 0.5 * er + 0.5 * ef - 1.0
    mult = lam64 + rho * c
    ref0 = float(df64.mean() - dr64.mean()) + lam64 * c + 0.5 * rho * c * c
    assert 0.3 < er < 3.0 and 0.3 < ef < 3.0
    assert abs(mult) >= 0.1 * (abs(lam64) + rho * abs(c))          # no case on a cancellation

    s = _lib.stream_handle(dev)
    nb = L.smmd_sobolev_workspace_bytes(br, bf, per)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    outs = [torch.empty(6, device=dev) for _ in range(2)]
    for out in outs:       # the second call on the same workspace: the ticket was left at rest
        _lib.check(L.smmd_sobolev_fwd(_lib.ptr(gr), _lib.ptr(gf), _lib.ptr(dr), _lib.ptr(df), br,
                                      bf, per, _lib.ptr(lam_t), rho, _lib.ptr(out), _lib.ptr(ws),
                                      nb, s), 'smmd_sobolev_fwd')
    assert torch.equal(outs[0], outs[1])
    got = outs[0].double().cpu().tolist()
    cb = 1e-5 * 0.5 * (er + ef)
    print('e_r %.6g e_f %.6g c %.6g mult %.6g; errors: e %.3g %.3g, c %.3g (cb %.3g), out0 %.3g, '
          'mult %.3g' % (er, ef, c, mult, abs(got[4] - er), abs(got[5] - ef), abs(got[2] - c), cb,
                         abs(got[0] - ref0), abs(got[3] - mult)))
    assert got[4] == pytest.approx(er, rel=1e-5) and got[5] == pytest.approx(ef, rel=1e-5)
    assert abs(got[2] - c) <= cb
    assert abs(got[3] - mult) <= rho * cb + 1e-6 * abs(mult)
    assert abs(got[0] - ref0) <= abs(mult) * cb + 0.5 * rho * cb * cb + 1e-6 * abs(ref0)
    assert got[1] == pytest.approx(-float(df64.mean()), rel=1e-5, abs=1e-7)

    go = torch.tensor([GO], device=dev)
    dgr, dgf = torch.empty_like(gr), torch.empty_like(gf)
    ddr, ddf = torch.empty(br, device=dev), torch.empty(bf, device=dev)
    _lib.check(L.smmd_sobolev_bwd(_lib.ptr(gr), _lib.ptr(gf), br, bf, per, _lib.ptr(outs[0]),
                                  _lib.ptr(go), _lib.ptr(dgr), _lib.ptr(dgf), _lib.ptr(ddr),
                                  _lib.ptr(ddf), s), 'smmd_sobolev_bwd')
    for got_dg, g64, b in ((dgr, gr64, br), (dgf, gf64, bf)):
        ref = GO * mult / b * g64                    # logical NCHW values either way
        assert ((got_dg.double().cpu() - ref).abs() <= 2e-5 * ref.abs()).all()
    assert torch.allclose(ddr.double().cpu(), torch.full((br,), -GO / br, dtype=torch.float64),
                          rtol=1e-6, atol=0)
    assert torch.allclose(ddf.double().cpu(), torch.full((bf,), GO / bf, dtype=torch.float64),
                          rtol=1e-6, atol=0)


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'unaligned'])
def test_decay_kernels(dev, shift):
    """Segments of 1, 3, 1024, 4097 and 5 elements packed back to back, a hole
    of 2 before the last (a segment of coefficient 0) and 3 elements past the
    table; the hole and the tail hold NaN, which nothing may read.  The 4097
    segment crosses the boundary of the two blocks."""
    from gan.core import _lib
    L = _lib.lib()
    offs = [0, 1, 4, 1028, 5125, 5127, 5132]
    coefs = [1e-6, 1e-3, 0.5, 2e-2, 0.0, 7.0]
    n = offs[-1] + 3
    buf = torch.randn(n + 1, generator=torch.Generator().manual_seed(5))
    buf[shift + 5125:shift + 5127] = float('nan')
    buf[shift + 5132:] = float('nan')
    w = buf.to(dev)[shift:shift + n]
    off_t = torch.tensor(offs, dtype=torch.int64, device=dev)
    cf_t = torch.tensor(coefs, device=dev)
    w64, cf64 = w.double().cpu(), cf_t.double().cpu()
    inside = [(a, b, float(cf)) for a, b, cf in zip(offs[:-1], offs[1:], cf64) if cf]
    ref = sum(cf * float((w64[a:b] ** 2).sum()) for a, b, cf in inside)
    ref_dw = torch.zeros(n, dtype=torch.float64)
    for a, b, cf in inside:
        ref_dw[a:b] = GO * 2.0 * cf * w64[a:b]

    s = _lib.stream_handle(dev)
    nb = L.smmd_decay_workspace_bytes(n)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    outs = [torch.empty(1, device=dev) for _ in range(2)]
    for out in outs:
        _lib.check(L.smmd_decay_fwd(_lib.ptr(w), n, _lib.ptr(off_t), _lib.ptr(cf_t), len(coefs),
                                    _lib.ptr(out), _lib.ptr(ws), nb, s), 'smmd_decay_fwd')
    assert torch.equal(outs[0], outs[1])
    assert float(outs[0]) == pytest.approx(ref, rel=1e-5)
    go = torch.tensor([GO], device=dev)
    dws = [torch.full((n + 1,), 3.0, device=dev)[shift:shift + n] for _ in range(2)]
    for dw in dws:
        _lib.check(L.smmd_decay_bwd(_lib.ptr(w), n, _lib.ptr(off_t), _lib.ptr(cf_t), len(coefs),
                                    _lib.ptr(go), _lib.ptr(dw), s), 'smmd_decay_bwd')
    assert torch.equal(dws[0], dws[1])
    got = dws[0].double().cpu()
    assert torch.allclose(got, ref_dw, rtol=1e-6, atol=0)
    assert (got[5125:5127] == 0).all() and (got[5132:] == 0).all()
