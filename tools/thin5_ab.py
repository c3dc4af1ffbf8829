"""A/B of the thin 5x5 stride-2 kernels (smmd_conv5s2_thin*) against MIOpen
(SMMD_THIN5=0's path) on the DCGAN 3-channel layers of the configs, at batch 64
and 128: the critics' first layer 3 -> 64 (pre-padded 35, 67, 163 -> 16, 32, 80)
and the generators' last layer 64 -> 3 (16, 32, 80 -> 32, 64, 160), each in its
three directions.  Event-timed, the two sides alternating in one process,
several rounds (median and spread reported).  `library_hbm_fraction` = the
bytes of the wide and the thin tensor over 8 TB/s (DESIGN.md's HBM figure) over
the library's time.

  python tools/thin5_ab.py [--batches 64,128] [--iters 50] [--rounds 5] [--out FILE]
writes profiles/thin5/thin5_ab_<source hash>.json (or FILE) and prints it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gan.core import _lib, convops  # noqa: E402

convops.THIN5 = convops.THIN5_ALL = True      # every layer and direction on the library's side

HBM_BYTES_PER_US = 8.0e6
CRITIC = [35, 67, 163]        # 3 -> 64, the pre-padded input size
GENERATOR = [16, 32, 80]      # 64 -> 3, the input size


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
    ap.add_argument('--batches', default='64,128')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('thin5_ab needs the GPU')
    dev = torch.device('cuda:0')
    aten = torch.ops.aten
    out = {'iters': a.iters, 'rounds': a.rounds, 'source': _lib.source_hash(),
           'device': torch.cuda.get_device_name(0), 'unit': 'us per call, median of rounds',
           'layers': []}
    for batch in (int(v) for v in a.batches.split(',')):
        for kind, sizes in (('critic 3->64', CRITIC), ('generator 64->3', GENERATOR)):
            for size in sizes:
                g = torch.Generator(device=dev).manual_seed(size)
                w = torch.randn(64, 3, 5, 5, device=dev, generator=g) / 9
                if kind.startswith('critic'):
                    thin = torch.randn(batch, 3, size, size, device=dev, generator=g)
                    d = convops._thin5_dims(thin.shape, w, (0, 0))
                    wide = torch.randn(batch, 64, d[5], d[6], device=dev, generator=g)
                    b = torch.randn(64, device=dev, generator=g)
                    assert convops._is_thin5(thin, w, (2, 2), (0, 0))

                    def mi(mask):
                        return lambda: aten.convolution_backward(
                            wide, thin, w, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1, mask)
                    sides = {
                        'conv': (lambda: convops._thin5_conv(thin, w, b, d),
                                 lambda: F.conv2d(thin, w, b, 2, 0)),
                        'convt': (lambda: convops._thin5_convt(wide, w, None, d),
                                  mi([True, False, False])),
                        'wgrad': (lambda: convops._thin5_wgrad(wide, thin, d),
                                  mi([False, True, False])),
                    }
                else:
                    wide = torch.randn(batch, 64, size, size, device=dev, generator=g)
                    d = convops._convt5_dims(wide, w)
                    thin = torch.randn(batch, 3, 2 * size, 2 * size, device=dev, generator=g)
                    b = torch.randn(3, device=dev, generator=g)
                    assert convops.convt5_thin_applicable(wide, w)
                    gpad = F.pad(thin, (0, 1, 0, 1))

                    def mi(mask):
                        return lambda: aten.convolution_backward(
                            gpad, wide, w, None, [2, 2], [1, 1], [1, 1], True, [0, 0], 1, mask)
                    sides = {
                        'convt': (lambda: convops._thin5_convt(wide, w, b, d),
                                  lambda: F.conv_transpose2d(wide, w, b, 2, 1)[:, :, :2 * size,
                                                                               :2 * size]),
                        'conv': (lambda: convops._thin5_conv(thin, w, None, d),
                                 mi([True, False, False])),
                        'wgrad': (lambda: convops._thin5_wgrad(wide, thin, d),
                                  mi([False, True, False])),
                    }
                floor = (wide.numel() + thin.numel()) * 4 / HBM_BYTES_PER_US
                rec = {'layer': kind, 'batch': batch, 'ct': 3, 'cw': 64, 'H': d[3], 'W': d[4],
                       'Ho': d[5], 'Wo': d[6], 'hbm_floor_us': floor}
                for name, (lib, ref) in sides.items():
                    tl, tr = [], []
                    for _ in range(a.rounds):
                        tl.append(timed(lib, a.iters))
                        tr.append(timed(ref, a.iters))
                    tl.sort()
                    tr.sort()
                    rec[name] = {'library_us': tl[len(tl) // 2], 'miopen_us': tr[len(tr) // 2],
                                 'library_spread_us': tl[-1] - tl[0],
                                 'miopen_spread_us': tr[-1] - tr[0],
                                 'library_hbm_fraction': floor / tl[len(tl) // 2],
                                 'miopen_hbm_fraction': floor / tr[len(tr) // 2]}
                out['layers'].append(rec)
                print(json.dumps(rec), flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'thin5', 'thin5_ab_%s.json' % out['source'])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
