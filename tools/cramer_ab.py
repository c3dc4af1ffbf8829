"""A/B of the fused Cramer loss side (SMMD_CRAMER_FUSED) at batch 64 and
dof_dim 1 / 16 / 256: the head, the seed and their backwards as one critic
update runs them (forward of both, then the backward of d_base + <U, W> for a
fixed W standing in for what the critic's double backward hands the seed), on
fixed critic outputs.  One process, interleaved rounds, medians of
event-timed loops; the launches and the summed kernel time per update come
from one profiled update per path.  Prints one JSON object and writes it to
argv[1] (default profiles/cramer/cramer_ab_<library stamp>.json).

    python tools/cramer_ab.py [out.json]
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
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from gan.core import _lib, ops  # noqa: E402

ROUNDS, ITERS, BATCH, DIMS = 9, 1000, 64, (1, 16, 256)


def main():
    dev = torch.device('cuda:0')
    out = {'workload': 'Cramer loss side per critic update (head + seed, forward and backward), '
                       'batch %d, variant cramer' % BATCH,
           'library': _lib.lib().smmd_source_hash().decode(), 'rounds': ROUNDS,
           'updates_per_round': ITERS, 'dof_dim': {}}
    for d in DIMS:
        gen = torch.Generator().manual_seed(d)
        g, g2, x, h = (torch.randn(BATCH, d, generator=gen).to(dev).requires_grad_(True)
                       for _ in range(4))
        w = torch.randn(BATCH, d, generator=gen).to(dev)

        def update(fused):
            ops.CRAMER_FUSED = fused
            d_base, _ = ops.cramer_head_loss(g, g2, x, 'cramer', want=1)
            U = ops.cramer_seed(h, g)
            torch.autograd.grad(d_base + (U * w).sum(), (g, g2, x, h))

        def timed(fused):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(ITERS):
                update(fused)
            e.record()
            torch.cuda.synchronize()
            return 1e3 * s.elapsed_time(e) / ITERS

        def profiled(fused):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                update(fused)
                torch.cuda.synchronize()
            ks = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
            return {'launches': len(ks), 'kernel_us': round(sum(ev.device_time for ev in ks), 2)}

        us = {True: [], False: []}
        for fused in (True, False):
            timed(fused)
        for _ in range(ROUNDS):
            for fused in (True, False):
                us[fused].append(timed(fused))
        rec = {}
        for fused, key in ((True, 'fused'), (False, 'plain')):
            rec[key] = dict(profiled(fused), us_per_update_median=round(
                statistics.median(us[fused]), 2), us_per_update_all=[round(v, 2) for v in us[fused]])
        out['dof_dim'][str(d)] = rec
    print(json.dumps(out))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, 'profiles', 'cramer', 'cramer_ab_%s.json' % out['library'])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
