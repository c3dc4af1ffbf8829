"""A/B of the FID's moments (SMMD_FID_COV) at the scorer's shape: mean and
covariance of 25 000 bootstrap-gathered rows of a 25 000 x 2048 code array.
Variant A is smmd_code_moments, variant B the float64 torch path on the device
(SMMD_FID_COV=0).  Interleaved rounds of event-timed calls, medians; the
library's error against the float64 path at that shape; one whole
fid_score(..., bootstrap, 3) with its host eigen time split out; and the errors
of the shapes tests/test_gpu_fid.py asserts on, which its bounds cite.  Prints
one JSON object and writes it to profiles/fid/fid_ab_<source hash>.json (or
argv[1]).

    python tools/fid_ab.py [out.json]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'scaled-mmd-gan_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gan import compute_scores as cs  # noqa: E402
from gan.core import _lib, fid  # noqa: E402

ROUNDS, CALLS, N, D = 7, 3, 25000, 2048
F32_MFMA_PEAK_TF = 157.3        # MI355X datasheet, dense f32 matrix


def test_errors(dev):
    """The figures behind COV_BOUND and FID_BOUND of tests/test_gpu_fid.py."""
    import test_fid_host as H
    import test_gpu_fid as T
    T.COV_BOUND = T.FID_BOUND = float('inf')         # measure, do not assert
    cov = {}
    for n, d in T.SHAPES:
        x = T.codes_for(n, d)
        index = np.random.default_rng(n + d).integers(0, n + 7, n).astype(np.int64)
        index[-1] = index[0]
        cov['(%d, %d) index None' % (n, d)] = T.check_moments(dev, x[:n], None, 'all rows')
        cov['(%d, %d) bootstrap' % (n, d)] = T.check_moments(dev, x, index, 'bootstrap')
    x = T.codes_for(257, 96, offset=1000.0)
    index = np.random.default_rng(9).integers(0, 264, 257).astype(np.int64)
    cov['(257, 96) + 1000 index None'] = T.check_moments(dev, x[:257], None, 'offset')
    cov['(257, 96) + 1000 bootstrap'] = T.check_moments(dev, x, index, 'offset bootstrap')
    fids, same = {}, {}
    for n, d, zeroed in H.CASES:
        g = H.make_codes(n, d, zeroed, 0.5)
        r = H.make_codes(n, d, zeroed, 0.4, seed_offset=1)
        want, ok = H.ref_fid_parts(g, r)
        assert ok
        G, R = torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev)
        got = cs.fid_score(G, R, splits=1, split_method='openai')[0]
        fids['(%d, %d)' % (n, d)] = abs(got - want) / abs(want)
        tr = 2 * np.trace(np.cov(g.astype(np.float64), rowvar=False))
        same['(%d, %d)' % (n, d)] = abs(cs.fid_score(G, G.clone(), splits=1,
                                                     split_method='openai')[0]) / tr
    g = H.make_codes(*H.CASES[1], 0.5)
    r = H.make_codes(*H.CASES[1], 0.4, seed_offset=1)
    np.random.seed(3)
    got = cs.fid_score(torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev), splits=2,
                       split_method='bootstrap')
    np.random.seed(3)
    want = cs.fid_score(torch.from_numpy(g), torch.from_numpy(r), splits=2,
                        split_method='bootstrap')
    fids['(200, 64) bootstrap vs float64 path'] = float((np.abs(got - want) / np.abs(want)).max())
    return {'cov_rel_err': cov, 'cov_rel_err_max': max(cov.values()),
            'fid_rel_err': fids, 'fid_rel_err_max': max(fids.values()),
            'fid_identical_sets_over_traces': same,
            'fid_identical_sets_max': max(same.values())}


def main():
    dev = torch.device('cuda:0')
    L = _lib.lib()
    out = {'library': L.smmd_source_hash().decode(), 'test_errors': test_errors(dev)}

    rng = np.random.default_rng(0)
    A = (rng.standard_normal((D, 64)) / 8).astype(np.float32)
    codes = torch.from_numpy(np.maximum(
        rng.standard_normal((N, 64)).astype(np.float32) @ A.T + 0.3, 0)).to(dev)
    ref = torch.from_numpy(np.maximum(
        rng.standard_normal((N, 64)).astype(np.float32) @ A.T + 0.25, 0)).to(dev)
    index = torch.from_numpy(rng.integers(0, N, N)).to(dev)

    def run(library, calls):
        os.environ['SMMD_FID_COV'] = '1' if library else '0'
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            res = fid.code_moments(codes, index)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / calls, res

    (_, (mean_a, cov_a)), (_, (mean_b, cov_b)) = run(True, 2), run(False, 2)
    ms = {True: [], False: []}
    for _ in range(ROUNDS):
        for library in (True, False):
            ms[library].append(run(library, CALLS)[0])
    med_a, med_b = statistics.median(ms[True]), statistics.median(ms[False])
    flops = 2.0 * N * D * D                     # the full product the float64 path forms
    out.update({
        'workload': 'code_moments of %d bootstrap rows of a %d x %d code array' % (N, N, D),
        'rounds': ROUNDS, 'calls_per_round': CALLS,
        'library_ms': {'median': round(med_a, 4), 'min': round(min(ms[True]), 4),
                       'all': [round(x, 4) for x in ms[True]]},
        'float64_torch_ms': {'median': round(med_b, 4), 'min': round(min(ms[False]), 4),
                             'all': [round(x, 4) for x in ms[False]]},
        'speedup_median': round(med_b / med_a, 3),
        'library_tflops_of_2nd2': round(flops / (med_a * 1e-3) / 1e12, 2),
        'library_tflops_executed_upper_triangle': round(
            flops * (528 * 64 * 64) / (D * D) / (med_a * 1e-3) / 1e12, 2),
        'f32_mfma_peak_tflops_datasheet': F32_MFMA_PEAK_TF,
        'workspace_bytes': int(L.smmd_code_moments_workspace_bytes(N, D)),
        'cov_rel_err_vs_float64_path': float((cov_a - cov_b).abs().max() / cov_b.abs().max()),
        'mean_rel_err_vs_float64_path': float((mean_a - mean_b).abs().max()
                                              / mean_b.abs().max()),
    })
    out['library_fraction_of_f32_mfma_peak'] = round(
        out['library_tflops_executed_upper_triangle'] / F32_MFMA_PEAK_TF, 3)

    # one whole fid_score, bootstrap, 3 splits; the host eigen step timed apart
    os.environ['SMMD_FID_COV'] = '1'
    eig = []
    inner = cs.frechet_distance

    def timed_fd(*a):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = inner(*a)
        eig.append(time.perf_counter() - t)
        return r
    cs.frechet_distance = timed_fd
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = cs.fid_score(codes, ref, split_method='bootstrap', splits=3)
    total = time.perf_counter() - t0
    cs.frechet_distance = inner
    out['fid_score_bootstrap_3'] = {'total_s': round(total, 3), 'host_eigen_s': round(sum(eig), 3),
                                    'rest_s': round(total - sum(eig), 3),
                                    'scores': [float(x) for x in scores]}
    print(json.dumps(out))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, 'profiles', 'fid', 'fid_ab_%s.json' % out['library'])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
