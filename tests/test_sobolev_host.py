"""The Sobolev GAN without a GPU: the tensor-op path of its two ops against
float64 autograd of the formulas (gan/core/sobolevgan_gp.py:16-42) written out,
the decay's segment table for the dcgan and snresnet critics, the dispatch."""
import os
import sys

import pytest

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# the oracle stands in for the optimizer's library; the small dcgan configuration
from test_gp_host import _cfg, fake  # noqa: E402,F401

CPU = torch.device('cpu')


@pytest.mark.parametrize('shape', [(2, 2, 3, 4, 4), (3, 2, 3, 5, 7)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_plain_head_matches_the_formulas(shape):
    from gan.core import ops
    br, bf, chw = shape[0], shape[1], tuple(shape[2:])
    gen = torch.Generator().manual_seed(0)

    def leaf(*s):
        return (0.2 * torch.randn(*s, generator=gen, dtype=torch.float64)).requires_grad_(True)
    dr, df, gr, gf = leaf(br, 1), leaf(bf, 1), leaf(br, *chw), leaf(bf, *chw)
    lam, rho, lam_t = -0.5, 10.0, torch.tensor([-0.5])
    d_base, g_loss, c, mult = ops.sobolev_head_loss(dr, df, gr, gf, lam_t, rho)
    e_r, e_f = (gr * gr).sum() / br, (gf * gf).sum() / bf
    ref_c = 0.5 * e_r + 0.5 * e_f - 1.0
    ref = df.mean() - dr.mean() + lam * ref_c + 0.5 * rho * ref_c * ref_c
    assert float(d_base.detach()) == pytest.approx(float(ref.detach()), rel=1e-12)
    assert float(g_loss) == pytest.approx(-float(df.mean()), rel=1e-12)
    assert float(c) == pytest.approx(float(ref_c), rel=1e-12)
    assert float(mult) == pytest.approx(lam + rho * float(ref_c), rel=1e-12)
    assert not (g_loss.requires_grad or c.requires_grad or mult.requires_grad)
    got = torch.autograd.grad(d_base, (dr, df, gr, gf))
    for a, b in zip(got, torch.autograd.grad(ref, (dr, df, gr, gf))):
        assert torch.allclose(a, b, rtol=1e-12, atol=0)


def test_plain_decay_matches_the_formulas():
    from gan.core import ops
    flat = torch.randn(40, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    offsets, coefs = torch.tensor([0, 12, 21, 40]), torch.tensor([1e-6, 1e-3, 0.5],
                                                                  dtype=torch.float64)
    # views of the buffer, one of them transposed (a channels-last weight's case)
    params = [flat[0:12].view(3, 4), torch.as_strided(flat, (3, 3), (1, 3), 12), flat[24:40]]
    params = [p.requires_grad_(True) for p in params]
    value = ops.weight_decay(params, flat, offsets, coefs)
    ref = 1e-6 * (flat[:12] ** 2).sum() + 1e-3 * (flat[12:21] ** 2).sum() \
        + 0.5 * (flat[24:40] ** 2).sum()
    assert float(value.detach()) == pytest.approx(float(ref), rel=1e-12)
    for g, p, cf in zip(torch.autograd.grad(value, params), params, (1e-6, 1e-3, 0.5)):
        assert torch.allclose(g, 2.0 * cf * p.detach(), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match='no one segment'):
        ops.weight_decay([flat[8:16]], flat, offsets, coefs)


@pytest.mark.parametrize('arch,kw', [('dcgan', {}), ('snresnet', dict(with_sn=True,
                                                                       with_learnable_sn_scale=True))])
def test_segment_table_and_dispatch(fake, arch, kw):  # noqa: F811
    from gan.core import snops
    from gan.core.smmd import get_model
    from gan.core.sobolevgan_gp import DECAY_CONV, DECAY_LINEAR, SobolevGAN, decay_table
    assert get_model('sobolev_gan') is SobolevGAN
    size = 32 if arch == 'snresnet' else 16
    m = SobolevGAN(_cfg(model='sobolev_gan', architecture=arch, output_size=size,
                        gradient_penalty=10.0, **kw), device=CPU)
    assert m.config.dof_dim == 1 and m.optim_name == 'sobolevgan10_loss'
    assert float(m.lam) == 0.0 and m.lam.shape == (1,)
    offsets, coefs = decay_table(m.discriminator, m.d_optim)
    assert offsets == m._decay_offsets.tolist()
    # the table covers the flat buffer exactly once, in ascending segments
    assert offsets[0] == 0 and offsets[-1] == m.d_optim.numel and offsets == sorted(set(offsets))
    per_element = torch.zeros(m.d_optim.numel)
    for a, b, cf in zip(offsets[:-1], offsets[1:], coefs):
        per_element[a:b] = cf
    final = [mod for mod in m.discriminator.modules() if isinstance(mod, snops.Linear)][-1]
    linear = {id(final.weight), id(final.bias)}
    for i, p in enumerate(m.d_optim.params):
        o = m.d_optim.offsets[i]
        want = DECAY_LINEAR if id(p) in linear else DECAY_CONV
        assert (per_element[o:o + p.numel()] == torch.tensor(want, dtype=torch.float32)).all()
    assert linear <= {id(p) for p in m.d_optim.params} and len(m.d_optim.params) > 2
    # the state carries the multiplier; a state without it loads as 0
    m.lam.fill_(0.75)
    sd = m.state_dict()
    m.lam.zero_()
    m.load_state_dict(sd)
    assert float(m.lam) == 0.75
    del sd['lam']
    m.load_state_dict(sd)
    assert float(m.lam) == 0.0
