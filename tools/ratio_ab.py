"""A/B of mmd.mmd2_and_ratio: the fused launches (smmd_mmd2_ratio_fwd / _bwd)
against SMMD_RATIO_FUSED=0 (three smmd_kernel_matrix launches, torch ops on
the N x N matrices and their autograd), forward + backward of the ratio, with
the mix_rq_1dot kernel at m in {64, 512, 2048} x d in {1, 16, 128}.
Interleaved rounds of event-timed calls on one device; medians and ranges.
Prints one JSON object and writes it, stamped with the library's source
hash, to profiles/ratio/ (or to argv[1]).

    python tools/ratio_ab.py [out.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gan.core import _lib, mmd  # noqa: E402

ROUNDS, WARMUP = 9, 5
SIZES = [(m, d) for m in (64, 512, 2048) for d in (1, 16, 128)]


def main():
    dev = torch.device('cuda:0')
    _lib.lib()
    rows = []
    for m, d in SIZES:
        calls = 40 if m <= 512 else 10
        g = torch.Generator(device='cpu').manual_seed(m * 1000 + d)
        X = torch.randn(m, d, generator=g).to(dev).requires_grad_(True)
        Y = (0.7 + 1.3 * torch.randn(m, d, generator=g)).to(dev).requires_grad_(True)

        def run(fused, n):
            os.environ['SMMD_RATIO_FUSED'] = '1' if fused else '0'
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                X.grad = Y.grad = None
                ratio = mmd.mmd2_and_ratio(mmd._mix_rq_1dot_kernel(X, Y))[1]
                ratio.backward()
            e.record()
            torch.cuda.synchronize()
            return 1e3 * s.elapsed_time(e) / n, ratio.item()

        # warm-up, and the values of both paths; smmd_kernel_matrix_fwd serves
        # d <= 32 only, so wider features have no materialised side
        vals = {True: run(True, WARMUP)[1]}
        try:
            vals[False] = run(False, WARMUP)[1]
        except _lib.SmmdError as err:
            vals[False] = str(err)
        sides = [f for f in (True, False) if not isinstance(vals[f], str)]
        us = {True: [], False: []}
        for _ in range(ROUNDS):
            for fused in sides:
                us[fused].append(run(fused, calls)[0])
        row = {'m': m, 'd': d, 'calls_per_round': calls,
               'ratio_fused': vals[True], 'ratio_materialised': vals[False]}
        for fused, key in ((True, 'fused_us'), (False, 'materialised_us')):
            if fused in sides:
                row[key] = {'median': round(statistics.median(us[fused]), 1),
                            'min': round(min(us[fused]), 1), 'max': round(max(us[fused]), 1)}
        row['workspace_bytes'] = int(_lib.lib().smmd_mmd2_ratio_workspace_bytes(m, d))
        row['materialised_matrix_bytes'] = 3 * m * m * 4
        rows.append(row)
        print(json.dumps(row), flush=True)
    stamp = _lib.lib().smmd_source_hash().decode()
    out = {'what': 'mmd2_and_ratio forward + backward of the ratio, mix_rq_1dot, per call '
                   '(host loop, device events around each round)',
           'library': stamp, 'rounds': ROUNDS, 'sizes': rows}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, 'profiles', 'ratio', 'ratio_ab_%s.json' % stamp)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
