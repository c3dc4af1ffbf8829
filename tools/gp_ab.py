"""A/B of the fused gradient-penalty loss side (SMMD_GP_FUSED) on the WGAN-GP
critic step: resnet5 64x64, width 64, batch 64, gp 10.  Interleaved rounds of
event-timed critic steps, medians; then the library's own event times of the
four entry points.  Prints one JSON object (and writes it to argv[1]).

    python tools/gp_ab.py [out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gan.core import _lib, ops  # noqa: E402
from gan.core.smmd import get_model  # noqa: E402
from gan.main import default_flags  # noqa: E402

ROUNDS, STEPS, BATCH = 9, 10, 64


def main():
    dev = torch.device('cuda:0')
    c = default_flags()
    c.update(dict(model='wgan_gp', architecture='resnet5', output_size=64, df_dim=64, gf_dim=64,
                  batch_size=BATCH, gradient_penalty=10.0, batch_norm=False, with_sn=False,
                  dataset='celebA'))
    torch.manual_seed(0)
    model = get_model('wgan_gp')(argparse.Namespace(**c), device=dev)
    images = torch.rand(BATCH, 3, 64, 64, device=dev)

    def run(fused, n):
        ops.GP_FUSED = fused
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            model.d_step(images)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n

    for fused in (True, False):
        run(fused, 5)
    ms = {True: [], False: []}
    for _ in range(ROUNDS):
        for fused in (True, False):
            ms[fused].append(run(fused, STEPS))
    _lib.enable_timing(True)
    _lib.reset_timing()
    run(True, STEPS)
    kernels = {k: {'calls': n, 'mean_us': round(1e3 * t, 2)}
               for k, (n, t) in _lib.timing_ms().items()
               if k.startswith('smmd_gp_') or k == 'smmd_critic_head_fwd'}
    _lib.enable_timing(False)
    out = {'workload': 'WGAN-GP critic step, resnet5 64x64, width 64, batch %d, gp 10' % BATCH,
           'library': _lib.lib().smmd_source_hash().decode(),
           'rounds': ROUNDS, 'steps_per_round': STEPS,
           'fused_ms_per_step': {'median': round(statistics.median(ms[True]), 4),
                                 'all': [round(x, 4) for x in ms[True]]},
           'plain_ms_per_step': {'median': round(statistics.median(ms[False]), 4),
                                 'all': [round(x, 4) for x in ms[False]]},
           'kernels_event_timed': kernels}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
