"""A/B of the wide 5x5 stride-2 transposed conv kernel (smmd_conv5s2t) against
MIOpen (SMMD_CONVT5=0's path: F.conv_transpose2d + the crop, a view; also
timed with the dense copy of it) on the wide
Deconv2d layers of the DCGAN generators at batch 64: dcgan at 32 and 64 px,
dcgan5 at 64 px (1024@2 -> 512@4 -> 256@8 -> 128@16 -> 64@32).  Event-timed, the
two sides alternating in one process after a warm-up of both, several rounds
(median and spread reported); the two outputs are compared at the timed size
first.  `library_mfma_fraction` = 2·25·N·h·w·cin·cout flops over 157 TFLOP/s
(DESIGN.md's f32 MFMA figure) over the library's time.  A shape enters
convops._CONVT5_FASTER when `faster_beyond_spread` is true.

  python tools/convt5_ab.py [--batch 64] [--iters 200] [--rounds 7] [--out FILE]
writes profiles/convt5/convt5_ab_<source hash>.json (or FILE) and prints it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gan.core import _lib, convops  # noqa: E402

convops.CONVT5 = convops.CONVT5_ALL = True      # every layer on the library's side

MFMA_FLOPS_PER_US = 157.0e6
# (cin, cout, h): the input of each wide layer
LAYERS = [(1024, 512, 2), (512, 256, 2), (512, 256, 4), (256, 128, 4), (256, 128, 8),
          (128, 64, 8), (128, 64, 16)]


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
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('convt5_ab needs the GPU')
    dev = torch.device('cuda:0')
    out = {'batch': a.batch, 'iters': a.iters, 'rounds': a.rounds, 'source': _lib.source_hash(),
           'device': torch.cuda.get_device_name(0), 'unit': 'us per call, median of rounds',
           'layers': []}
    for cin, cout, h in LAYERS:
        g = torch.Generator(device=dev).manual_seed(cin + h)
        x = torch.randn(a.batch, cin, h, h, device=dev, generator=g)
        w = torch.randn(cin, cout, 5, 5, device=dev, generator=g) / (5 * cin ** 0.5)
        b = torch.randn(cout, device=dev, generator=g)
        assert convops.convt5_applicable(x, w)

        def lib():
            return convops._convt5(x, w, b)

        def ref():                              # the crop is a view: no copy on this side
            return F.conv_transpose2d(x, w, b, 2, 1)[:, :, :2 * h, :2 * h]

        def ref_copy():                         # with the dense copy a consumer may make
            return ref().contiguous()
        yl, yr = lib(), ref()
        diff = ((yl - yr).abs().max() / yr.abs().max()).item()
        tl, tr, tc = [], [], []
        for _ in range(a.rounds):
            tl.append(timed(lib, a.iters))
            tr.append(timed(ref, a.iters))
            tc.append(timed(ref_copy, a.iters))
        tl.sort()
        tr.sort()
        tc.sort()
        ml, mr = tl[len(tl) // 2], tr[len(tr) // 2]
        flops = 2 * 25 * a.batch * h * h * cin * cout
        rec = {'cin': cin, 'cout': cout, 'h': h, 'w': h, 'library_us': ml, 'miopen_us': mr,
               'miopen_copy_us': tc[len(tc) // 2], 'library_spread_us': tl[-1] - tl[0],
               'miopen_spread_us': tr[-1] - tr[0],
               'library_mfma_fraction': flops / MFMA_FLOPS_PER_US / ml,
               'workspace_bytes': _lib.lib().smmd_conv5s2t_workspace_bytes(a.batch, cin, cout, h, h),
               'max_rel_diff_vs_miopen': diff,
               'faster_beyond_spread': tl[-1] < tr[0]}
        out['layers'].append(rec)
        print(json.dumps(rec), flush=True)
    path = a.out or os.path.join(ROOT, 'profiles', 'convt5', 'convt5_ab_%s.json' % out['source'])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
