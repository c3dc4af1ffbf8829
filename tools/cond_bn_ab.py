"""A/B of SMMD_COND_BN on one GPU: a cond_snresnet critic step and generator
step (64x64, batch 64, configs' widths) with the library's conditional batch
norm + ReLU (1) against the torch ops (0).

One process, one model; the switch (snops.COND_BN) alternates between rounds
in the order 1 0 0 1 ..., so clock and thermal drift fall on both sides.  Each
round times `--steps` steps of one kind between two device syncs after
`--warmup` untimed ones.  Prints one JSON line: per kind and side the median
per-step time over the rounds with the lowest and highest round.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--num_classes', type=int, default=1000)
    a = ap.parse_args()
    import torch
    from gan.core import miopen_db, snops
    from gan.core.smmd import SMMD
    from gan.main import default_flags
    miopen_db.install()
    c = default_flags()
    c.update(dict(batch_size=64, output_size=64, architecture='cond_snresnet', with_labels=True,
                  num_classes=a.num_classes, kernel='rbf', model='smmd', batch_norm=True,
                  with_sn=True, with_learnable_sn_scale=True, with_scaling=True, dof_dim=1,
                  df_dim=64, gf_dim=64, dataset='imagenet'))
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = SMMD(argparse.Namespace(**c), device=dev)
    images = torch.rand(64, 3, 64, 64, device=dev)
    labels = torch.randint(0, a.num_classes, (64,), device=dev)
    times = {(k, s): [] for k in ('d_step', 'g_step') for s in (1, 0)}
    order = [1, 0, 0, 1]
    for r in range(a.rounds):
        side = order[r % 4]
        snops.COND_BN = bool(side)
        for kind in ('d_step', 'g_step'):
            step = getattr(model, kind)
            for _ in range(a.warmup):
                step(images, labels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(images, labels)
            torch.cuda.synchronize()
            times[(kind, side)].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {'shape': 'cond_snresnet 64x64 batch 64 width 64, %d classes' % a.num_classes,
           'rounds_per_side': a.rounds // 2, 'steps_per_round': a.steps}
    for (kind, side), v in times.items():
        out['%s_ms_cond_bn_%d' % (kind, side)] = {
            'median': round(statistics.median(v), 3), 'min': round(min(v), 3),
            'max': round(max(v), 3)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
