"""The C-ABI library loads and exports every symbol include/smmd_hip.h
declares; host-only entry points (workspace sizing, argument validation,
status strings) behave without a GPU."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'smmd_hip.h')


def _declared():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(smmd_[a-z0-9_]+)\s*\(', src)))


@pytest.fixture(scope='module')
def L():
    from gan.core import _lib
    return _lib.lib()


def test_header_and_binding_agree():
    from gan.core import _lib
    assert _declared() == sorted(_lib.EXPORTED_SYMBOLS)


def test_every_declared_symbol_is_exported(L):
    for name in _declared():
        assert hasattr(L, name), name


def test_status_strings(L):
    from gan.core import _lib
    assert L.smmd_status_string(0) == b'SMMD_OK'
    assert b'EINVAL' in L.smmd_status_string(1)
    assert L.smmd_abi_version() == _lib.ABI_VERSION == 17


def test_workspace_sizing(L):
    from gan.core import _lib
    assert L.smmd_mmd2_workspace_bytes(64, 64, 1) >= 256            # one-block path
    assert L.smmd_mmd2_workspace_bytes(2048, 2048, 1) >= 256 + (4096 // 8) * 8 * 8
    assert L.smmd_scaled_loss_workspace_bytes(64, 3 * 64 * 64) >= 64 * 3 * 8
    arr = (_lib.SnLayer * 2)()
    arr[0].N, arr[0].K, arr[1].N, arr[1].K = 64, 27, 1024, 4608
    assert L.smmd_sn_workspace_bytes(arr, 2) > 16 * 4608 * 4
    offs = (ctypes.c_int64 * 3)(0, 10, 70000)
    assert L.smmd_opt_workspace_bytes(offs, 2) >= 8 * 6
    # the weight gradients' slice partials, and past 32 slices the scratch of
    # the group level behind them: 36 slices in groups of 16 / 16 / 4 (stride
    # 2), 33 in 16 / 16 / 1 (3x3, tile rows of 6: the first form's dU slabs)
    assert L.smmd_wino4x4s2_wgrad_workspace_bytes(9, 16, 64, 64, 64) == (36 + 3) * 64 * 16 * 16 * 4
    assert L.smmd_wino3x3_wgrad_workspace_bytes(8, 64, 64, 88, 12) == (33 + 3) * 64 * 64 * 16 * 4


def test_argument_validation_without_gpu(L):
    from gan.core import _lib
    d = _lib.KernelDesc()
    d.kind, d.n_terms, d.param[0], d.wt[0] = 0, 1, 1.0, 1.0
    # NULL inputs / bad ranges are rejected before any launch
    assert L.smmd_mmd2_fwd(d, None, 4, None, 4, 1, 0, 0, 4, 0, 4, None, None, None, None, None,
                           0, None) == 1
    bad = _lib.KernelDesc()
    bad.kind, bad.n_terms = 0, 0
    x = ctypes.c_void_p(16)
    assert L.smmd_mmd2_fwd(bad, x, 4, x, 4, 1, 0, 0, 4, 0, 4, None, None, None, None, x, 1 << 20,
                           None) == 1
    assert L.smmd_mmd2_fwd(d, x, 4, x, 4, 1, 0, 0, 5, 0, 4, None, None, None, None, x, 1 << 20,
                           None) == 1
    assert L.smmd_mmd2_fwd(d, x, 4, x, 4, 1, 0, 0, 4, 0, 4, None, None, None, None, x, 8,
                           None) == 3          # EWORKSPACE
    # d > 32 takes the MFMA Gram path, whose workspace holds the padded Z and
    # the coefficient matrix: one byte short of the query is rejected
    small = L.smmd_mmd2_workspace_bytes(4, 4, 32)
    wide = L.smmd_mmd2_workspace_bytes(4, 4, 64)
    assert wide >= 256 + 64 * 64 * 4 * 2 > small
    assert L.smmd_mmd2_fwd(d, x, 4, x, 4, 64, 0, 0, 4, 0, 4, None, None, None, None, x, wide - 1,
                           None) == 3          # EWORKSPACE
    assert L.smmd_sn_power_iter(None, 0, 1, 1e-12, 1, None, 0, None) == 1
    arr = (_lib.SnLayer * 1)()
    arr[0].N, arr[0].K = 4, 4
    assert L.smmd_sn_power_iter_ex(arr, 1, 1, 1e-12, 1, 2, x, 1 << 20, None) == 1   # bad flag
    offs = (ctypes.c_int64 * 3)(0, 16, 32)
    idx = (ctypes.c_int32 * 1)(5)                                 # tensor index out of range
    assert L.smmd_adam_flat_sn(x, x, x, x, offs, 2, 1.0, 1.0, 1e-4, 0.5, 0.9, 1e-8, 1, x,
                               1 << 20, arr, idx, 1, x, 1 << 20, None) == 1
    idx2 = (ctypes.c_int32 * 2)(1, 1)                             # one tensor twice
    arr2 = (_lib.SnLayer * 2)()
    assert L.smmd_adam_flat_sn(x, x, x, x, offs, 2, 1.0, 1.0, 1e-4, 0.5, 0.9, 1e-8, 1, x,
                               1 << 20, arr2, idx2, 2, x, 1 << 20, None) == 1
    big = (ctypes.c_int64 * 98)(*range(0, 98 * 4, 4))            # > 96 tensors: unsupported
    assert L.smmd_adam_flat_sn(x, x, x, x, big, 97, 1.0, 1.0, 1e-4, 0.5, 0.9, 1e-8, 1, x,
                               1 << 20, arr, (ctypes.c_int32 * 1)(0), 1, x, 1 << 20, None) == 4
    assert L.smmd_witness_bwd(d, x, 4, x, 4, x, 4, 1, None, x, x, x, None) == 1
    # Winograd 3x3: shapes it does not tile, missing operands, a short workspace
    assert L.smmd_wino3x3_supported(64, 64, 64, 64, 64) == 1
    assert L.smmd_wino3x3_supported(64, 60, 64, 64, 64) == 0       # ci % 8
    assert L.smmd_wino3x3_supported(64, 64, 96, 64, 64) == 0       # ko % 64
    assert L.smmd_wino3x3_supported(64, 64, 64, 63, 64) == 0       # odd height
    assert L.smmd_wino3x3_filter(x, 96, 64, 0, x, 1 << 30, None) == 4
    assert L.smmd_wino3x3_filter(x, 64, 64, 2, x, 1 << 30, None) == 1
    assert L.smmd_wino3x3_filter(x, 64, 64, 0, x, 16 * 64 * 64 * 4 - 1, None) == 3
    assert L.smmd_wino3x3_conv(None, x, None, x, 2, 8, 64, 4, 4, None, 0, None) == 1
    assert L.smmd_wino3x3_conv(x, x, None, x, 2, 8, 64, 5, 4, None, 0, None) == 4
    need = L.smmd_wino3x3_workspace_bytes(64, 512, 512, 8, 8)       # split input channels
    assert need >= 2 * 64 * 512 * 64 * 4
    assert L.smmd_wino3x3_conv(x, x, None, x, 64, 512, 512, 8, 8, x, need - 1, None) == 3
    assert L.smmd_wino3x3_workspace_bytes(64, 64, 64, 64, 64) == 0
    # polyphase 4x4 stride-2: tiling limits and argument checks before any launch
    assert L.smmd_wino4x4s2_supported(64, 64, 128, 64, 64) == 1
    assert L.smmd_wino4x4s2_supported(64, 3, 128, 64, 64) == 0     # ci odd
    assert L.smmd_wino4x4s2_supported(64, 64, 96, 64, 64) == 0     # ko % 64
    assert L.smmd_wino4x4s2_supported(64, 64, 128, 66, 64) == 0    # h % 4
    assert L.smmd_wino4x4s2t_supported(64, 128, 64, 32, 32) == 1
    assert L.smmd_wino4x4s2t_supported(64, 12, 64, 32, 32) == 0    # k % 8
    assert L.smmd_wino4x4s2t_supported(64, 128, 96, 32, 32) == 0   # c % 64
    assert L.smmd_wino4x4s2_filter_bytes(128, 64) == 36 * 128 * 64 * 4
    assert L.smmd_wino4x4s2_filter(x, 96, 64, x, 1 << 30, None) == 4
    assert L.smmd_wino4x4s2t_filter(x, 128, 96, x, 1 << 30, None) == 4
    assert L.smmd_wino4x4s2_filter(x, 128, 64, x, 36 * 128 * 64 * 4 - 1, None) == 3
    assert L.smmd_wino4x4s2_conv(None, x, None, x, 2, 8, 64, 4, 4, None, 0, None) == 1
    assert L.smmd_wino4x4s2_conv(x, x, None, x, 2, 8, 64, 6, 4, None, 0, None) == 4
    assert L.smmd_wino4x4s2t_conv(x, x, None, x, 2, 8, 64, 3, 4, None, 0, None) == 4
    need = L.smmd_wino4x4s2_workspace_bytes(64, 512, 1024, 8, 8)
    assert need >= 2 * 64 * 1024 * 16 * 4
    assert L.smmd_wino4x4s2_conv(x, x, None, x, 64, 512, 1024, 8, 8, x, need - 1, None) == 3


def test_conservative_variant_exports_every_symbol():
    """The conservative LDS-DMA build (`make conservative`, or
    SMMD_BUILD_CONSERVATIVE=1 with __graft_entry__.build(); tooling only:
    tools/lib_bitexact.py compares it with the shipped one bit for bit on the
    GPU) loads and exports the same ABI -- checked when it is as new as the
    shipped library (a stale one from an earlier build is not a product file)."""
    path = os.path.join(ROOT, 'scaled-mmd-gan_amd', 'lib', 'libsmmd_hip_dmasync.so')
    main = os.path.join(ROOT, 'scaled-mmd-gan_amd', 'lib', 'libsmmd_hip.so')
    if not os.path.exists(path) or os.path.getmtime(path) < os.path.getmtime(main):
        pytest.skip('conservative variant not built for this tree '
                    '(make -C scaled-mmd-gan_amd/csrc conservative)')
    C = ctypes.CDLL(path)
    for name in _declared():
        assert hasattr(C, name), name


def test_wino_supported_2gib_boundary(L):
    """The Winograd kernels address x and y through buffer descriptors whose
    range is 0x7fffffff bytes (2^31 = the out-of-range sentinel): every
    tensor must stay under 2^29 floats, and `supported` says 0 at the edge."""
    # 3x3: x = n ci h w, y = n ko h w floats
    assert L.smmd_wino3x3_supported(1, 8, 64, 2048, 4096 - 2) == 1           # y just under 2^29
    assert L.smmd_wino3x3_supported(1, 8, 64, 2048, 4096) == 0               # y = 2^29
    assert L.smmd_wino3x3_supported(1, 64, 64, 2048, 4096) == 0              # x = 2^29
    # stride 2: x = n ci h w, y = n ko h w / 4
    assert L.smmd_wino4x4s2_supported(1, 8, 64, 4096, 8192 - 4) == 1
    assert L.smmd_wino4x4s2_supported(1, 8, 64, 4096, 8192) == 0            # y = 2^29
    assert L.smmd_wino4x4s2_supported(1, 32, 64, 4096, 4096) == 0           # x = 2^29
    # transposed: gy = n k hg wg, dx = 4 n c hg wg
    assert L.smmd_wino4x4s2t_supported(1, 8, 64, 1024, 2048 - 2) == 1
    assert L.smmd_wino4x4s2t_supported(1, 8, 64, 1024, 2048) == 0           # dx = 2^29
    assert L.smmd_wino4x4s2t_supported(1, 256, 64, 1024, 2048) == 0         # gy = 2^29
    # 3x3 weight gradient: one image's 64-channel range under 2 GiB
    assert L.smmd_wino3x3_wgrad_supported(1, 64, 64, 2048, 4096 - 4) == 1
    assert L.smmd_wino3x3_wgrad_supported(1, 64, 64, 2048, 4096) == 0
    # the Python routing helper holds the same bound
    from gan.core import convops

    class _T:
        def __init__(self, shape):
            self.shape = shape

        def numel(self):
            n = 1
            for s in self.shape:
                n *= s
            return n
    assert convops._under_2g(_T((1, 8, 2048, 4094)), 64)
    assert not convops._under_2g(_T((1, 8, 2048, 4096)), 64)
    assert not convops._under_2g(_T((1, 64, 2048, 4096)), 1)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, 'scaled-mmd-gan_amd')
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith('.py'):
                src = open(os.path.join(dp, f)).read()
                assert 'oracle' not in re.findall(r'^\s*(?:from|import)\s+(\w+)', src, re.M), f


def test_library_stamp_matches_sources(L, monkeypatch):
    """The .so carries the hash of the sources it was built from; a binary
    older than csrc/ + include/ is refused at load (never silently run)."""
    from gan.core import _lib
    assert L.smmd_source_hash().decode() == _lib.source_hash()
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'source_hash', lambda: '0' * 16)
    with pytest.raises(_lib.SmmdLibraryError, match='other sources'):
        _lib.lib()
