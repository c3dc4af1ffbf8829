"""smmd_conv5s2t without a GPU: the shape rule holds for every wide Deconv2d
layer of the DCGAN generators at batch 64 (dcgan at 32 and 64 px, dcgan5 at 64
px) and the argument checks answer before any launch."""
import ctypes

import pytest

torch = pytest.importorskip('torch')

# (cin, cout, h): 1024@2 -> 512@4 -> 256@8 -> 128@16 -> 64@32 and the 32 px stack
GENERATOR = [(1024, 512, 2), (512, 256, 2), (512, 256, 4), (256, 128, 4), (256, 128, 8),
             (128, 64, 8), (128, 64, 16)]


@pytest.fixture(scope='module')
def L():
    from gan.core import _lib
    return _lib.lib()


@pytest.mark.parametrize('cin,cout,h', GENERATOR)
def test_generator_shapes_supported(L, cin, cout, h):
    assert L.smmd_conv5s2t_supported(64, cin, cout, h, h) == 1


def test_cout_off_the_64_multiple_unsupported(L):
    assert L.smmd_conv5s2t_supported(64, 128, 48, 16, 16) == 0
    x = ctypes.c_void_p(16)
    assert L.smmd_conv5s2t(x, x, None, x, 64, 128, 48, 16, 16, None, 0, None) == 4


def test_null_pointer_and_short_workspace_are_einval(L):
    d = (2, 512, 64, 2, 2)                      # one tile: the channel split
    need = L.smmd_conv5s2t_workspace_bytes(*d)
    assert need > 0
    x = ctypes.c_void_p(16)
    assert L.smmd_conv5s2t(None, x, None, x, *d, x, need, None) == 1
    assert L.smmd_conv5s2t(x, None, None, x, *d, x, need, None) == 1
    assert L.smmd_conv5s2t(x, x, None, None, *d, x, need, None) == 1
    assert L.smmd_conv5s2t(x, x, None, x, *d, x, need - 1, None) == 1
    assert L.smmd_conv5s2t(x, x, None, x, *d, None, 0, None) == 1
