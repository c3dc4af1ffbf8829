"""KID (polynomial-kernel MMD) and FID scoring of gan/compute_scores.py on the
MI355X.

Mirrors the reference's ``polynomial_mmd_averages`` (:211-229),
``polynomial_mmd`` (:232-243) and ``_mmd2_and_variance`` (:246-335): same
arguments, same numpy return values.  The three m x m kernel matrices are
never formed: ``smmd_poly_kernel_sums`` evaluates them tile by tile on the
f32 matrix cores and keeps only their row/column sums, diagonals and squared
sums; the estimator and its variance run in double on the device.

``get_splits`` (:159-166) and ``fid_score`` (:180-208) are the reference's
too: each split's mean and covariance come from ``smmd_code_moments``
(gan/core/fid.py), which reads the split's rows of the device-resident codes
in place, and the d x d spectral step runs in float64 on the host.

The Inception featurizer and inception_score need the Inception graph, which
the reference downloads (:22-39) and which is unavailable offline: callers
pass codes (e.g. synthetic [n, 2048] pool3 features), and the command line
below takes code arrays only:

    python scaled-mmd-gan_amd/gan/compute_scores.py CODES.npy \\
        --reference-feats REF.npy [--do-fid|--no-fid] [--do-mmd|--no-mmd] \\
        [--splits N] [--split-method openai|bootstrap] [--mmd-subsets N] \\
        [--mmd-subset-size N] [--output out.npz]
"""
from __future__ import annotations

import os
import sys

if __name__ == '__main__' and not __package__:      # run as a script: become gan.compute_scores
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gan.compute_scores import main as _main
    sys.exit(_main())

import numpy as np
import torch

from .core import _lib
from .core.fid import code_moments, frechet_distance
from .core.mmd import PolySums, _codes, poly_mmd2_and_variance, polynomial_kernel_sums


def polynomial_mmd_averages(codes_g, codes_r, n_subsets=50, subset_size=1000, ret_var=True,
                            output=sys.stdout, **kernel_args):
    """KID over random subsets, drawn as the reference does (np.random.choice
    without replacement, :220-222); codes stay on the GPU between subsets."""
    m = min(codes_g.shape[0], codes_r.shape[0])
    mmds = np.zeros(n_subsets)
    if ret_var:
        vars_ = np.zeros(n_subsets)
    choice = np.random.choice
    G = _codes(codes_g)
    R = _codes(codes_r, G.device)
    for i in range(n_subsets):
        gi = torch.from_numpy(choice(len(codes_g), subset_size, replace=False)).to(G.device)
        ri = torch.from_numpy(choice(len(codes_r), subset_size, replace=False)).to(G.device)
        o = polynomial_mmd(G.index_select(0, gi), R.index_select(0, ri), var_at_m=m,
                           ret_var=ret_var, **kernel_args)
        if ret_var:
            mmds[i], vars_[i] = o
        else:
            mmds[i] = o
    return (mmds, vars_) if ret_var else mmds


def polynomial_mmd(codes_g, codes_r, degree=3, gamma=None, coef0=1, var_at_m=None,
                   ret_var=True):
    """k(x, y) = (gamma <x, y> + coef0)^degree, gamma = 1/dim by default."""
    X = _codes(codes_g)
    Y = _codes(codes_r, X.device)
    kw = dict(degree=degree, gamma=gamma, coef0=coef0)
    xx = polynomial_kernel_sums(X, X, **kw)
    yy = polynomial_kernel_sums(Y, Y, **kw)
    xy = polynomial_kernel_sums(X, Y, **kw)
    mmd2, var = poly_mmd2_and_variance(xx, yy, xy, var_at_m=var_at_m).tolist()
    return (mmd2, var) if ret_var else mmd2


def _sums_of_matrix(K):
    K = K.to(dtype=torch.float64)
    d = torch.diagonal(K)
    stats = torch.stack([K.sum(), (K * K).sum(), d.sum(), (d * d).sum()])
    return PolySums(K.sum(1).contiguous(), K.sum(0).contiguous(), d.contiguous(),
                    stats.contiguous(), tuple(K.shape))


def _mmd2_and_variance(K_XX, K_XY, K_YY, unit_diagonal=False, mmd_est='unbiased',
                       block_size=1024, var_at_m=None, ret_var=True):
    """The reference's estimator on already-formed kernel matrices (:246-335),
    reduced on the device.  unit_diagonal: the diagonals are taken as 1."""
    mats = [torch.as_tensor(np.asarray(k) if not torch.is_tensor(k) else k) for k in
            (K_XX, K_XY, K_YY)]
    dev = torch.device('cuda', torch.cuda.current_device())
    mats = [k.to(dev) for k in mats]
    m = mats[0].shape[0]
    assert all(k.shape == (m, m) for k in mats)
    if unit_diagonal:
        for k in (0, 2):
            mats[k] = mats[k].clone()
            mats[k].fill_diagonal_(1.0)
    xx, xy, yy = (_sums_of_matrix(k) for k in mats)
    mmd2, var = poly_mmd2_and_variance(xx, yy, xy, var_at_m=var_at_m, mmd_est=mmd_est).tolist()
    return (mmd2, var) if ret_var else mmd2


def get_splits(n, splits=10, split_method='openai'):
    """The reference's splits (:159-166): contiguous slices, or bootstrap
    draws from the global numpy stream."""
    if split_method == 'openai':
        edges = [i * n // splits for i in range(splits + 1)]
        return [slice(a, b) for a, b in zip(edges, edges[1:])]
    if split_method == 'bootstrap':
        return [np.random.choice(n, n) for _ in range(splits)]
    raise ValueError('bad split_method %r' % (split_method,))


def _fid_codes(x, device=None):
    """float32 codes where the moments will run: a torch tensor stays on its
    device (CPU tensors take code_moments' float64 path); an array goes to the
    GPU once (``_codes``), or stays on the host where there is none."""
    if device is None and torch.is_tensor(x) and not x.is_cuda:
        device = x.device
    if device is None and not torch.is_tensor(x) and not torch.cuda.is_available():
        device = torch.device('cpu')
    return _codes(x, device)


def _split_moments(codes, w):
    if isinstance(w, slice):
        return code_moments(codes[w])                    # a view: rows are contiguous
    return code_moments(codes, torch.from_numpy(np.asarray(w, dtype=np.int64)))


def fid_score(codes_g, codes_r, eps=1e-6, output=sys.stdout, **split_args):
    """FID per split (:180-208) as a numpy array of ``splits`` scores.  The
    codes go to the device once; each split hands its slice or bootstrap index
    to ``code_moments`` (no gathered copy).  ``eps`` is unused: the eigenvalue
    form of the trace term (``frechet_distance``) is defined on singular
    covariances, so the reference's retry (:200-203) has nothing to do; it is
    kept for the signature.  ``output`` took the reference's progress bar."""
    splits_g = get_splits(codes_g.shape[0], **split_args)
    splits_r = get_splits(codes_r.shape[0], **split_args)
    assert len(splits_g) == len(splits_r)
    d = codes_g.shape[1]
    assert codes_r.shape[1] == d
    G = _fid_codes(codes_g)
    R = _fid_codes(codes_r, G.device)
    scores = np.zeros(len(splits_g))
    for i, (w_g, w_r) in enumerate(zip(splits_g, splits_r)):
        mn_g, cov_g = _split_moments(G, w_g)
        mn_r, cov_r = _split_moments(R, w_r)
        scores[i] = frechet_distance(mn_g, cov_g, mn_r, cov_r)
    return scores


def main(argv=None):
    """Scores of saved code arrays (the reference's :338-390 options that do
    not need the Inception graph)."""
    import argparse
    parser = argparse.ArgumentParser(description='FID / KID of two [n, d] code arrays (.npy)')
    parser.add_argument('samples', help='codes of the samples, .npy [n, d]')
    parser.add_argument('--reference-feats', required=True, help='reference codes, .npy [m, d]')
    parser.add_argument('--output', '-o')
    g = parser.add_mutually_exclusive_group()
    g.add_argument('--do-fid', action='store_true', default=True)
    g.add_argument('--no-fid', action='store_false', dest='do_fid')
    g = parser.add_mutually_exclusive_group()
    g.add_argument('--do-mmd', action='store_true', default=False)
    g.add_argument('--no-mmd', action='store_false', dest='do_mmd')
    parser.add_argument('--mmd-subsets', type=int, default=100)
    parser.add_argument('--mmd-subset-size', type=int, default=1000)
    parser.add_argument('--splits', type=int, default=10)
    parser.add_argument('--split-method', choices=['openai', 'bootstrap'], default='bootstrap')
    parser.add_argument('--device', default=None,
                        help="where the moments run: 'cuda' (default where there is one) or 'cpu'")
    args = parser.parse_args(argv)
    if args.output and os.path.exists(args.output):
        parser.error("Path {} already exists".format(args.output))
    if args.output and os.path.dirname(args.output):
        os.makedirs(os.path.dirname(args.output), exist_ok=True)

    codes = np.load(args.samples)
    ref = np.load(args.reference_feats)
    if codes.ndim != 2 or ref.ndim != 2 or codes.shape[1] != ref.shape[1]:
        parser.error('need two [n, d] arrays of one width (got %s and %s)' % (codes.shape,
                                                                             ref.shape))
    to_save = {}
    if args.do_fid:
        if args.device is not None:
            dev = torch.device(args.device)
            codes_f, ref_f = _codes(codes, dev), _codes(ref, dev)
        else:
            codes_f, ref_f = codes, ref
        scores = fid_score(codes_f, ref_f, splits=args.splits, split_method=args.split_method)
        print("FID mean:", np.mean(scores))
        print("FID std:", np.std(scores))
        to_save['fid'] = scores
    if args.do_mmd:
        mmd2s = polynomial_mmd_averages(codes, ref, n_subsets=args.mmd_subsets,
                                        subset_size=args.mmd_subset_size, ret_var=False)
        print("KID mean:", mmd2s.mean())
        print("KID std:", mmd2s.std())
        to_save['mmd2'] = mmd2s
    if args.output:
        np.savez(args.output, **to_save)
    return 0


__all__ = ['polynomial_mmd_averages', 'polynomial_mmd', '_mmd2_and_variance', 'get_splits',
           'fid_score', 'main', '_lib']
