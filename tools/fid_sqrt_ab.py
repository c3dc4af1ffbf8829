"""A/B of the FID's spectral step at the scorer's shape: frechet_distance on
the moments of 25 000 bootstrap-gathered rows of two 25 000 x 2048 code arrays,
spectral='host' (two float64 eigh on the CPU, after copying the covariances
there) against spectral='device' (smmd_fid_trace_sqrt: Newton-Schulz products
on the f64 matrix cores).  Interleaved rounds after a warm-up of both; a call
is timed by the host clock from a synchronised device to its returned float
(both paths end in a read-back).  The library call alone is event-timed for the
executed f64 TF/s.  Also |device - host| over the traces, the residuals, and
one whole fid_score(..., bootstrap, 3) per path.  Prints one JSON object and
writes it to profiles/fid_sqrt/fid_sqrt_ab_<source hash>.json (or argv[1]).

    python tools/fid_sqrt_ab.py [out.json]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gan import compute_scores as cs  # noqa: E402
from gan.core import _lib, fid  # noqa: E402

ROUNDS, N, D = 5, 25000, 2048
EVENT_CALLS = 3
F64_MFMA_PEAK_TF = 78.6         # MI355X datasheet, f64 matrix
BT, KC = 128, 8                 # csrc/smmd_fid_sqrt.hip: block tile, k chunk


def executed_flops(d, iters):
    """MFMA flops of one smmd_fid_trace_sqrt: per stage 3 products an
    iteration less the last Z, and the residual's; two for M.  Every product
    runs whole tiles and whole k chunks."""
    products = 2 * (3 * iters - 1 + 1) + 2          # 314 at 52 iterations
    side = -(-d // BT) * BT
    return products, products * 2.0 * side * side * (-(-d // KC) * KC)


def main():
    dev = torch.device('cuda:0')
    L = _lib.lib()
    out = {'library': L.smmd_source_hash().decode()}

    rng = np.random.default_rng(0)
    A = (rng.standard_normal((D, 64)) / 8).astype(np.float32)
    codes = torch.from_numpy(np.maximum(
        rng.standard_normal((N, 64)).astype(np.float32) @ A.T + 0.3, 0)).to(dev)
    ref = torch.from_numpy(np.maximum(
        rng.standard_normal((N, 64)).astype(np.float32) @ A.T + 0.25, 0)).to(dev)
    mg, cg = fid.code_moments(codes, torch.from_numpy(rng.integers(0, N, N)).to(dev))
    mr, cr = fid.code_moments(ref, torch.from_numpy(rng.integers(0, N, N)).to(dev))
    traces = float(torch.trace(cg) + torch.trace(cr))

    def run(spectral):
        torch.cuda.synchronize()
        t = time.perf_counter()
        score = fid.frechet_distance(mg, cg, mr, cr, spectral=spectral)
        return time.perf_counter() - t, score

    scores = {k: run(k)[1] for k in ('device', 'host')}           # warm-up of both
    out4 = fid.trace_sqrt(cg, cr).tolist()
    assert out4[1] <= fid.SQRT_RESIDUAL_MAX and out4[2] <= fid.SQRT_RESIDUAL_MAX, out4
    secs = {'host': [], 'device': []}
    for _ in range(ROUNDS):
        for k in ('host', 'device'):
            secs[k].append(run(k)[0])

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(EVENT_CALLS):
        fid.trace_sqrt(cg, cr)
    e.record()
    torch.cuda.synchronize()
    lib_ms = s.elapsed_time(e) / EVENT_CALLS
    iters = fid.sqrt_iters(fid.SQRT_DELTA)
    products, flops = executed_flops(D, iters)
    tf = flops / (lib_ms * 1e-3) / 1e12
    med = {k: statistics.median(v) for k, v in secs.items()}
    out.update({
        'workload': 'frechet_distance on the moments of %d bootstrap rows of two %d x %d code '
                    'arrays (one split)' % (N, N, D),
        'rounds': ROUNDS, 'delta': fid.SQRT_DELTA, 'iters': iters,
        'host_s_per_split': {'median': round(med['host'], 4),
                             'all': [round(x, 4) for x in secs['host']]},
        'device_s_per_split': {'median': round(med['device'], 4),
                               'all': [round(x, 4) for x in secs['device']]},
        'host_over_device_median': round(med['host'] / med['device'], 3),
        'smmd_fid_trace_sqrt_ms': round(lib_ms, 3),
        'products': products, 'executed_f64_tflop': round(flops / 1e12, 3),
        'executed_f64_tflops': round(tf, 2),
        'f64_mfma_peak_tflops_datasheet': F64_MFMA_PEAK_TF,
        'fraction_of_f64_mfma_peak': round(tf / F64_MFMA_PEAK_TF, 3),
        'workspace_bytes': int(L.smmd_fid_trace_sqrt_workspace_bytes(D)),
        'score_host': scores['host'], 'score_device': scores['device'],
        'abs_diff_over_traces': abs(scores['device'] - scores['host']) / traces,
        'residual_stage1': out4[1], 'residual_stage3': out4[2],
    })

    whole = {}
    for k in ('host', 'device'):
        np.random.seed(0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        sc = cs.fid_score(codes, ref, split_method='bootstrap', splits=3, spectral=k)
        whole[k] = {'total_s': round(time.perf_counter() - t, 3), 'scores': [float(x) for x in sc]}
    out['fid_score_bootstrap_3'] = whole

    print(json.dumps(out))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, 'profiles', 'fid_sqrt', 'fid_sqrt_ab_%s.json' % out['library'])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
