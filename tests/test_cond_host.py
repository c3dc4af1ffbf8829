"""Class-conditional training without a GPU: the cond_snresnet pair
(architecture.py:71-100, :291-320 of the reference), conditional batch norm +
ReLU on its plain-tensor path against the formula in float64
(resnet/ops/cond_batchnorm.py:6-17, resnet/block.py:42-47), the model's label
plumbing and guards, the flags, the labelled TFRecord pipeline on shards
written here, and the library's argument checks."""
import argparse
import ctypes
import io
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

K = 5


@pytest.fixture
def fake(monkeypatch):
    """The oracle stands in for the library where a CPU model needs it (the
    optimizer, the SN bank), as in tests/test_gp_host.py."""
    import fake_lib
    from gan.core import _lib, sn
    f = fake_lib.FakeLib()
    monkeypatch.setattr(sn, 'SN_FOLD', False)       # the bank's fold launch is GPU-only
    monkeypatch.setattr(_lib, '_lib', f)
    monkeypatch.setattr(_lib, 'lib', lambda: f)
    monkeypatch.setattr(_lib, 'require_cuda', lambda *t: None)
    monkeypatch.setattr(_lib, 'stream_handle', lambda device=None: None)
    monkeypatch.setattr(_lib, 'workspace', lambda tag, nbytes, device: torch.zeros(
        max(int(nbytes), 256), dtype=torch.uint8))
    return f


def _cfg(**kw):
    from gan.main import default_flags
    c = default_flags()
    c.update(dict(batch_size=4, output_size=64, architecture='cond_snresnet', with_labels=True,
                  num_classes=K, kernel='rbf', model='smmd', batch_norm=True, with_sn=True,
                  with_learnable_sn_scale=True, with_scaling=True, dof_dim=3, df_dim=4, gf_dim=4,
                  learning_rate=1e-4, dataset='imagenet'))
    c.update(kw)
    return argparse.Namespace(**c)


def test_get_networks_returns_the_pair():
    from gan.core import architecture as A
    G, D = A.get_networks('cond_snresnet')
    assert G is A.CondSNResNetGenerator and D is A.CondProjectionSNResNetDiscriminator
    for name in ('d-fullconv5', 'dc64', 'dcgan64', 'dc128'):
        with pytest.raises(NotImplementedError):
            A.get_networks(name)


@pytest.mark.parametrize('size,blocks', [(64, 4), (32, 5)])
def test_output_shapes(size, blocks):
    from gan.core import architecture as A
    from gan.core.snops import CondBatchNorm2d
    torch.manual_seed(0)
    G_cls, D_cls = A.get_networks('cond_snresnet')
    G = G_cls(K, 4, 3, size, True, z_dim=16)
    D = D_cls(K, 4, 3, False, input_size=size)
    assert len(G.res) == blocks and len(D.res) == blocks
    norms = [m for m in G.modules() if isinstance(m, CondBatchNorm2d)]
    assert len(norms) == 2 * blocks
    assert isinstance(G.bn4, torch.nn.BatchNorm2d)          # g_h4 stays unconditional
    for bn in norms:
        assert bn.scale.shape == bn.offset.shape == (K, bn.C)
        assert torch.equal(bn.scale, torch.ones(K, bn.C))
        assert torch.equal(bn.offset, torch.zeros(K, bn.C))
        assert not list(bn.buffers())
    y = torch.tensor([0, 4, 2])
    with torch.no_grad():
        img = G(torch.rand(3, 16) * 2 - 1, y)
    assert img.shape == (3, 3, size, size)
    assert 0.0 <= float(img.min()) and float(img.max()) <= 1.0
    assert D(img, y=y).shape == (3, 3)
    layers = D(img, return_layers=True, y=y)
    assert layers['hF'].shape == (3, 3) and 'h4' in layers
    with pytest.raises(ValueError):
        G(torch.rand(3, 16), None)


def test_existing_block_calls_unchanged():
    """block(x) of the unconditional modes takes no labels and gives what it
    gave; a conditional block without labels is an error, not a silent norm."""
    from gan.core import architecture as A
    torch.manual_seed(0)
    x = torch.randn(2, 8, 4, 4)
    b = A.ResidualBlock(8, 4, 3, 'up', 'batchnorm')
    assert b(x).shape == (2, 4, 8, 8)
    c = A.ResidualBlock(8, 4, 3, 'up', 'cond_batchnorm', num_classes=K)
    assert c(x, torch.tensor([1, 3])).shape == (2, 4, 8, 8)
    with pytest.raises(ValueError):
        c(x)
    with pytest.raises(ValueError):
        A.ResidualBlock(8, 4, 3, 'up', 'cond_batchnorm')


def test_projection_term():
    """hF(y) - hF(None) is exactly sum_j (w_y * hF(None))_j, w_y the rows y of
    the embedding (architecture.py:315-318)."""
    from gan.core import architecture as A
    torch.manual_seed(1)
    D = A.CondProjectionSNResNetDiscriminator(K, 4, 3, False, input_size=64)
    assert D.embed.weight.shape == (3, K)                   # kept as Linear keeps it
    assert 0.005 < float(D.embed.weight.detach().std()) < 0.02       # normal init, std 0.01
    with torch.no_grad():
        D.embed.weight.mul_(30.0)
    x = torch.rand(4, 3, 64, 64)
    y = torch.tensor([4, 0, 0, 2])
    with torch.no_grad():
        plain = D(x)
        with_y = D(x, y=y)
        w_y = D.embed.weight.t()[y]
    assert torch.equal(with_y, plain + (w_y * plain).sum(1, keepdim=True))
    assert float((with_y - plain).abs().max()) > 1e-6
    with torch.no_grad():
        lay, lay_y = D(x, return_layers=True), D(x, return_layers=True, y=y)
    assert torch.equal(lay['hF'], plain) and torch.equal(lay_y['hF'], with_y)
    assert torch.equal(lay['h4'], lay_y['h4'])


def _cond_bn_relu_64(x, scale, offset, y, eps=1e-5):
    x, scale, offset = x.double(), scale.double(), offset.double()
    mean = x.mean((0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((0, 2, 3), keepdim=True)
    z = (x - mean) / torch.sqrt(var + eps) * scale[y][:, :, None, None] \
        + offset[y][:, :, None, None]
    return torch.relu(z)


@pytest.mark.parametrize('shape', [(5, 7, 4, 4), (3, 2, 2, 3)])
def test_cond_bn_relu_cpu_matches_float64(shape):
    from gan.core.snops import CondBatchNorm2d, cond_bn_relu
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g) * 3 + 1).requires_grad_(True)
    gy = torch.randn(shape, generator=g)
    bn = CondBatchNorm2d(K, shape[1])
    with torch.no_grad():
        bn.scale.copy_(torch.rand(K, shape[1], generator=g) + 0.5)
        bn.offset.copy_(torch.randn(K, shape[1], generator=g))
    y = torch.randint(0, K, (shape[0],), generator=g)
    out = cond_bn_relu(bn, x, y)
    out.backward(gy)
    x64 = x.detach().double().requires_grad_(True)
    s64 = bn.scale.detach().double().requires_grad_(True)
    o64 = bn.offset.detach().double().requires_grad_(True)
    ref = _cond_bn_relu_64(x64, s64, o64, y)
    ref.backward(gy.double())
    assert float((out.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6
    for got, want in ((x.grad, x64.grad), (bn.scale.grad, s64.grad), (bn.offset.grad, o64.grad)):
        assert float((got.double() - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-6
    # int32 labels (what the generator hands every layer) select the same rows
    with torch.no_grad():
        assert torch.equal(cond_bn_relu(bn, x, y.to(torch.int32)), out)
    with pytest.raises(ValueError):
        cond_bn_relu(bn, x, None)


def test_labels_cast_once_per_forward(monkeypatch):
    from gan.core import architecture as A
    from gan.core import snops
    calls = []
    real = snops.labels_int32

    def counting(y):
        calls.append(y.dtype)
        return real(y)
    monkeypatch.setattr(A, 'labels_int32', counting)
    seen = []
    real_op = A.cond_bn_relu
    monkeypatch.setattr(A, 'cond_bn_relu', lambda bn, x, y: seen.append(y.dtype) or real_op(bn, x, y))
    G = A.CondSNResNetGenerator(K, 4, 3, 64, True, z_dim=16)
    G(torch.rand(2, 16), torch.tensor([1, 2]))
    assert calls == [torch.int64]
    assert seen == [torch.int32] * 8


def test_model_builds_and_registers_the_embedding(fake):
    from gan.core.smmd import SMMD
    from gan.core.snops import sn_modules
    torch.manual_seed(0)
    m = SMMD(_cfg(), device=torch.device('cpu'))
    assert m.with_labels and m.num_classes == K
    emb = m.discriminator.embed
    assert emb in sn_modules(m.discriminator)
    assert any(e.module is emb for e in m.sn_D.entries)
    ids = {id(p) for p in m.d_optim.params}
    assert id(emb.weight) in ids and id(emb.sn_scale) in ids
    for bn in m.generator.modules():
        if hasattr(bn, 'offset'):
            gids = {id(p) for p in m.g_optim.params}
            assert id(bn.scale) in gids and id(bn.offset) in gids
    y = m.sample_y(64)
    assert y.shape == (64,) and int(y.min()) >= 0 and int(y.max()) < K
    assert m.get_samples(5).shape == (5, 3, 64, 64)
    sd = m.state_dict()
    assert 'embed.weight' in sd['D'] and any(k.endswith('bn1.scale') for k in sd['G'])
    # the default: the reference's 1000 classes (model.py:83)
    c = _cfg()
    del c.num_classes
    assert SMMD(c, device=torch.device('cpu')).num_classes == 1000


def test_tower_loss_uses_both_label_sets(fake):
    from gan.core.smmd import SMMD
    torch.manual_seed(0)
    m = SMMD(_cfg(), device=torch.device('cpu'))
    with torch.no_grad():
        m.discriminator.embed.weight.mul_(30.0)
    m.sn_D.refresh(update_u=False)
    g = torch.Generator().manual_seed(2)
    images, fake_im = torch.rand(4, 3, 64, 64, generator=g), torch.rand(4, 3, 64, 64, generator=g)
    la, lb = torch.tensor([0, 1, 2, 3]), torch.tensor([4, 4, 0, 1])
    m.set_tower_loss(images, fake_im, False, labels=la, fake_labels=lb)
    assert m.labels is la and m.y is lb
    D = m.discriminator
    with torch.no_grad():
        assert torch.allclose(m.d_images.detach(), D(images, y=la))
        assert torch.allclose(m.d_G.detach(), D(fake_im, y=lb))
        assert not torch.allclose(D(images, y=la), D(images, y=lb))
    with pytest.raises(ValueError):
        m.set_tower_loss(images, fake_im, False)
    with pytest.raises(ValueError):
        m.set_tower_loss(images, fake_im, False, labels=la)


def test_guards(fake):
    from gan.core.smmd import SMMD
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='with_labels'):
        SMMD(_cfg(architecture='snresnet'), device=cpu)             # labels, other networks
    with pytest.raises(ValueError, match='with_labels'):
        SMMD(_cfg(with_labels=False), device=cpu)                    # the networks, no labels
    with pytest.raises(NotImplementedError, match='global'):
        SMMD(_cfg(), device=cpu, dp_mode='global')
    m = SMMD(_cfg(), device=cpu)
    with pytest.raises(NotImplementedError, match='graphs'):
        m.enable_graphs(True)
    m.enable_graphs(False)
    images = torch.rand(4, 3, 64, 64)
    for step in (m.d_step, m.g_step, m.train_step):
        with pytest.raises(ValueError, match='labels'):
            step(images)                                             # a missing label
        with pytest.raises(ValueError, match='outside'):
            step(images, labels=torch.tensor([0, 1, K, 2]))          # out of range
        with pytest.raises(ValueError, match='outside'):
            step(images, labels=torch.tensor([0, -1, 1, 2]))
    plain = SMMD(_cfg(architecture='snresnet', with_labels=False), device=cpu)
    with pytest.raises(ValueError, match='labels'):
        plain.d_step(images, labels=torch.tensor([0, 1, 2, 3]))


def test_flags_parse():
    from gan.main import build_parser, default_flags
    d = default_flags()
    assert d['with_labels'] is False and d['num_classes'] == 1000
    f = build_parser().parse_args(['-with_labels', 'true', '-num_classes', '7',
                                   '-architecture', 'cond_snresnet'])
    assert f.with_labels is True and f.num_classes == 7


def test_main_hands_labels_to_the_pipeline(tmp_path):
    from gan import main as M
    f = argparse.Namespace(**dict(M.default_flags(), dataset='cifar10', with_labels=True))
    with pytest.raises(ValueError, match='with_labels'):
        M.make_pipeline(f, 32, 3, torch.device('cpu'))

    class P1:
        def next(self):
            return 'images'

    class P2:
        def next(self):
            return 'images', 'labels'
    assert M.next_batch(P1()) == ('images', None)
    assert M.next_batch(P2()) == ('images', 'labels')


def _jpeg(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format='JPEG', quality=95)
    return b.getvalue()


def _labelled_shards(root, labels_per_shard):
    """Flat-colour 256x256 JPEGs whose grey level is 40 * label."""
    from gan.core import pipeline as P
    d = root / 'tf_records_train'
    d.mkdir()
    n = len(labels_per_shard)
    for s, labels in enumerate(labels_per_shard):
        recs = []
        for lab in labels:
            a = np.full((256, 256, 3), 40 * (lab % 6), np.uint8)
            recs.append(P.encode_example({'image/encoded': _jpeg(a), 'image/height': 256,
                                          'image/width': 256, 'image/format': b'JPEG',
                                          'image/class/label': lab}))
        P.write_tfrecords(str(d / ('train-%05d-of-%05d' % (s, n))), recs)


def test_pipeline_yields_labels(tmp_path):
    from gan.core import pipeline as P
    _labelled_shards(tmp_path, [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]])
    P.DataFlow.buffer_size = 4
    try:
        pipe = P.ImagenetDataFlow(64, 3, 6, str(tmp_path), device='cpu', workers=2, verify=True,
                                  with_labels=True, num_classes=K)
        batches = [pipe.next() for _ in range(3)]
        pipe.stop()
        plain = P.ImagenetDataFlow(64, 3, 6, str(tmp_path), device='cpu', workers=2)
        x = plain.next()
        plain.stop()
    finally:
        P.DataFlow.buffer_size = 4000
    assert torch.is_tensor(x) and x.shape == (6, 3, 64, 64)       # unlabelled: as before
    for images, labels in batches:
        assert images.shape == (6, 3, 64, 64) and images.dtype == torch.float32
        assert labels.shape == (6,) and labels.dtype == torch.int64
        # each label travels with its own image
        grey = images.mean((1, 2, 3)) * 255.0
        assert torch.allclose(grey, 40.0 * labels.float(), atol=2.0)
    assert len({int(v) for _, l in batches for v in l}) > 1


def test_pipeline_names_the_shard_of_a_bad_label(tmp_path):
    from gan.core import pipeline as P
    _labelled_shards(tmp_path, [[0, 1, 2, 3], [1, 2, K, 0]])
    P.DataFlow.buffer_size = 2
    try:
        pipe = P.ImagenetDataFlow(64, 3, 4, str(tmp_path), device='cpu', workers=2,
                                  with_labels=True, num_classes=K)
        with pytest.raises(RuntimeError) as e:
            for _ in range(4):
                pipe.next()
        pipe.stop()
    finally:
        P.DataFlow.buffer_size = 4000
    cause = e.value.__cause__
    assert isinstance(cause, ValueError)
    assert 'train-00001-of-00002' in str(cause) and 'outside [0, %d)' % K in str(cause)
    with pytest.raises(ValueError, match='somewhere'):
        P.check_label_range(-1, K, 'somewhere')
    assert P.check_label_range(K - 1, K, 'x') == K - 1


def test_library_argument_checks():
    from gan.core import _lib
    L = _lib.lib()
    x = ctypes.c_void_p(4096)
    N, C, HW = 4, 8, 16
    assert L.smmd_cond_bn_relu_workspace_bytes(0, 8) == 0
    need = L.smmd_cond_bn_relu_workspace_bytes(N, C)
    assert need >= N * C * 2 * 8 + C * 2 * 8                       # ab and one statistics slab
    fwd = [x, x, N, C, HW, K, x, x, 1e-5, x, x, x, need, None]
    bwd = [x, x, x, N, C, HW, K, x, x, x, x, x, x, x, need, None]
    # every call below is refused before any launch (x is not a real buffer)
    for i in (0, 1, 6, 7, 9, 11):                                   # x, labels, scale, offset, y, ws
        a = list(fwd)
        a[i] = None
        assert L.smmd_cond_bn_relu_fwd(*a) == 1, i
    for i in (0, 1, 2, 7, 8, 9, 10, 11, 12, 13):
        a = list(bwd)
        a[i] = None
        assert L.smmd_cond_bn_relu_bwd(*a) == 1, i
    for i, v in ((2, 0), (3, 0), (4, 6), (4, 0), (5, 0), (5, -3), (12, need - 1)):
        a = list(fwd)
        a[i] = v
        assert L.smmd_cond_bn_relu_fwd(*a) == 1, (i, v)
    for i, v in ((3, 0), (4, 0), (5, 6), (6, 0), (6, -1), (14, need - 1)):
        a = list(bwd)
        a[i] = v
        assert L.smmd_cond_bn_relu_bwd(*a) == 1, (i, v)
    odd = ctypes.c_void_p(4100)                                     # not 16-byte aligned
    assert L.smmd_cond_bn_relu_fwd(*([odd] + fwd[1:])) == 1
