"""A/B of the 5x5 stride-2 convolution kernels (smmd_conv5s2*) against MIOpen
(SMMD_CONV5=0's path;
`library_mfma_fraction` = 2 * 25 * pixels * cin * cout flops over the 157.3 TF/s f32
MFMA peak) on the four wide DCGAN5 critic layers at batch 64:
event-timed forward, input gradient and weight gradient, the two sides
alternating in one process, several rounds (their spread is reported).

  python tools/conv5_ab.py [--batch 64] [--iters 50] [--rounds 5] [--out FILE]
writes profiles/conv5/conv5_ab_<source hash>.json (or FILE) and prints it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gan.core import _lib, convops  # noqa: E402

convops.CONV5_ALL = True          # every layer and direction on the library's side

LAYERS = [(64, 128, 32), (128, 256, 16), (256, 512, 8), (512, 1024, 4)]   # cin, cout, image


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('conv5_ab needs the GPU')
    dev = torch.device('cuda:0')
    aten = torch.ops.aten
    out = {'batch': a.batch, 'iters': a.iters, 'rounds': a.rounds, 'source': _lib.source_hash(),
           'device': torch.cuda.get_device_name(0), 'unit': 'us per call, median of rounds',
           'layers': []}
    for ci, co, hw in LAYERS:
        g = torch.Generator(device=dev).manual_seed(ci)
        x = torch.randn(a.batch, ci, hw + 3, hw + 3, device=dev, generator=g)   # pre-padded
        w = torch.randn(co, ci, 5, 5, device=dev, generator=g) / (5 * ci ** 0.5)
        b = torch.randn(co, device=dev, generator=g)
        gy = torch.randn(a.batch, co, hw // 2, hw // 2, device=dev, generator=g)
        pad = (0, 0)
        assert convops._is_k5s2(x, w, (2, 2), pad)

        def mi(mask):
            return lambda: aten.convolution_backward(gy, x, w, None, [2, 2], [0, 0], [1, 1],
                                                     False, [0, 0], 1, mask)
        sides = {
            'fwd': (lambda: convops._k5s2_conv(x, w, b, pad),
                    lambda: F.conv2d(x, w, b, 2, 0)),
            'dx': (lambda: convops._k5s2_dx(gy, w, x.shape, pad), mi([True, False, False])),
            'wgrad': (lambda: convops._k5s2_wgrad(gy, x, pad), mi([False, True, False])),
        }
        rec = {'cin': ci, 'cout': co, 'image': hw, 'gflop': 2e-9 * 25 * a.batch * (hw // 2) ** 2 * ci * co}
        for name, (lib, ref) in sides.items():
            tl, tr = [], []
            for _ in range(a.rounds):
                tl.append(timed(lib, a.iters))
                tr.append(timed(ref, a.iters))
            tl.sort()
            tr.sort()
            rec[name] = {'library_us': tl[len(tl) // 2], 'miopen_us': tr[len(tr) // 2],
                         'library_spread_us': tl[-1] - tl[0], 'miopen_spread_us': tr[-1] - tr[0],
                         'library_mfma_fraction': rec['gflop'] * 1e6 / tl[len(tl) // 2] / 157.3e3}
        out['layers'].append(rec)
    path = a.out or os.path.join(ROOT, 'profiles', 'conv5', 'conv5_ab_%s.json' % out['source'])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
