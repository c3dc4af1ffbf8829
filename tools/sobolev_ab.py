"""A/B of the fused Sobolev loss side (SMMD_SOBOLEV_FUSED) as one critic update
runs it: the head on fixed critic outputs and input gradients (batch 64,
64x64x3), the weight decay over the snresnet critic's parameter list in a
FlatAdam buffer, and the backward of their sum.  One process, interleaved
rounds, medians of event-timed loops; the launches and the summed kernel time
per update come from one profiled update per path, and the fused path's
library calls are listed by their _lib.timed names.  Prints one JSON object
and writes it to argv[1] (default profiles/sobolev/sobolev_ab_<library
stamp>.json).

    python tools/sobolev_ab.py [out.json]
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
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from gan.core import _lib, ops  # noqa: E402
from gan.core.architecture import get_networks  # noqa: E402
from gan.core.optim import FlatAdam  # noqa: E402
from gan.core.sobolevgan_gp import decay_table  # noqa: E402
from gan.main import default_flags  # noqa: E402

ROUNDS, ITERS, BATCH, SIZE = 9, 300, 64, 64


def main():
    dev = torch.device('cuda:0')
    c = argparse.Namespace(**default_flags())
    torch.manual_seed(0)
    D = get_networks('snresnet')[1](c.df_dim, 1, False, with_sn=True,
                                    with_learnable_sn_scale=False, input_size=SIZE).to(dev)
    params = [p for p in D.parameters() if p.requires_grad]
    opt = FlatAdam(params, 1e-4, name='D')
    offsets, coefs = decay_table(D, opt)
    off_t = torch.tensor(offsets, dtype=torch.int64, device=dev)
    cf_t = torch.tensor(coefs, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(1)
    scale = (1.0 / (3 * SIZE * SIZE)) ** 0.5
    g_real, g_fake = ((scale * torch.randn(BATCH, 3, SIZE, SIZE, generator=gen)).to(dev)
                      .requires_grad_(True) for _ in range(2))
    d_real, d_fake = (torch.randn(BATCH, 1, generator=gen).to(dev).requires_grad_(True)
                      for _ in range(2))
    lam = torch.full((1,), 0.25, device=dev)
    leaves = [d_real, d_fake, g_real, g_fake] + params

    def update(fused):
        ops.SOBOLEV_FUSED = fused
        d_base = ops.sobolev_head_loss(d_real, d_fake, g_real, g_fake, lam, 10.0)[0]
        torch.autograd.grad(d_base + ops.weight_decay(params, opt.flat_param, off_t, cf_t), leaves)

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

    out = {'workload': 'Sobolev loss side per critic update (head + decay, forward and backward), '
                       'batch %d at %dx%dx3, snresnet critic: %d tensors, %d floats'
                       % (BATCH, SIZE, SIZE, len(params), opt.numel),
           'library': _lib.lib().smmd_source_hash().decode(), 'rounds': ROUNDS,
           'updates_per_round': ITERS}
    us = {True: [], False: []}
    for fused in (True, False):
        timed(fused)
    for _ in range(ROUNDS):
        for fused in (True, False):
            us[fused].append(timed(fused))
    for fused, key in ((True, 'fused'), (False, 'plain')):
        out[key] = dict(profiled(fused), us_per_update_median=round(statistics.median(us[fused]), 2),
                        us_per_update_all=[round(v, 2) for v in us[fused]])
    _lib.reset_timing()
    _lib.enable_timing(True)
    update(True)
    out['fused']['library_calls'] = {k: n for k, (n, _) in _lib.timing_ms().items()}
    _lib.enable_timing(False)
    print(json.dumps(out))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, 'profiles', 'sobolev', 'sobolev_ab_%s.json' % out['library'])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
