"""Every width and row count of the witness op and the materialised kernel
matrix (csrc/smmd_mmd.hip: witness_fwd_kernel, witness_bwd_h_kernel,
witness_bwd_z_kernel, kmat_fwd_kernel, kmat_bwd_kernel) against the float64
autograd reference oracle/torch_kernels.py, through
``gan.core.mmd.witness_and_grad`` and ``gan.core.mmd.kernel_matrix``.

Inputs are seeded float32 (standard normal / sqrt(d), so that pair distances
stay O(1) at every width); the reference sees the same values widened.

Bounds
  w, K                1e-5 + 1e-4 |ref|
  dH, gA, gB          1e-4 max|ref| + 1e-3 |ref|   (test_gpu_parity._grad_close)
  gH, gR, gF          2e-3 max|ref| + 2e-3 |ref|   (the second-order bound of
                      test_gpu_parity.test_witness_second_order)

Conditioning.  Each case's reference is evaluated twice, plain and with
``raw32=True`` (the Gram expansion also rounded as fp32 rounds it); a case is
kept only if the two agree within a quarter of every bound above.
``test_conditioning_caps`` (no GPU) recomputes that for every case, asserts
that the cases failing it are exactly ``DROPPED``, and that their share is 0
for the rbf / rq / dot kinds and at most 1 in 10 for distance /
tanh_distance.  Seeds derive from the case id.  Rows of one side are redrawn
until they are 0.02 away from every row of the other side (``_apart``): at a
coincident pair the clamp max(raw, 0) has a kink, and the side of 0 on which
fp32 rounds raw switches an O(1) second-order term.

Dropped: ``wit-width-distance-5x70x9-d1`` alone.  On a line the distance
kernel sqrt((h - r)^2 + 1e-5) is almost linear, its second order is what is
left after be and b1 (h - r)^2 cancel, and the fp32 rounding of raw moves
gH / gR / gF by 5 - 10 quarter-bounds at every one of 40 seeds.  The same
kernel instantiation (DT = 1, distance) is reached by
``wit-width-tanh_distance-5x70x9-d1``, where tanh bends the line; that case is
moved to its ninth seed (``SEED_BUMP``), the first at which it is well
conditioned with a margin of 2.

(kernel, DT) -> a value-checked case, DT = 1, 2, 4, 8, 16, 32 from
d = 1, 2, 3|5 -> 4|8, 8|13 -> 8|16, 16|17 -> 16|32, 31|32:
  witness_fwd_kernel<DT>, witness_bwd_h_kernel<DT>, witness_bwd_z_kernel<DT>
      test_witness[width-<name>-5x70x9-d<d>]  for each of the four kinds
      (rbf: rbf, mix_rbf; rq: mix_rq*; distance: distance, tanh_distance; dot)
  kmat_fwd_kernel<DT>, kmat_bwd_kernel<DT, side 0 and 1>
      test_kernel_matrix[width-<name>-19x70-d<d>]
  grid stride (rows > 8192): test_witness[stride-...], test_kernel_matrix[stride-...]
  lane stride (> 64 columns): the width cases (70 columns) and rows-*-3x130x65,
      rows-*-70x3x129, rows-*-5x65, rows-*-130x3

Worst observed error as a share of its bound on an MI355X, per kernel kind
(the tests print it per case as ``worst``), with the error and max|ref| of
that case:
  kind      w, K                  first order           second order
  rbf       0.083 (1.2e-6, 0.18)  0.001 (1.6e-6, 12.7)  5e-5 (1.0e-7, 0.98)
  rq        0.109 (1.2e-6, 0.21)  0.004 (4.6e-7, 0.23)  0.002 (4.3e-7, 0.11)
  distance  0.041 (1.8e-6, 3.8)   0.013 (3.3e-5, 13.5)  0.073 (1.3e-6, 8.0e-3)
  dot       0.005 (1.3e-7, 1.8)   0.006 (1.6e-6, 0.22)  < 1e-3 (1.9e-12, 2.4e-5)
The second-order bound is left at the project's 2e-3: the distance kind uses
7 % of it, the others far less.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import smmd_oracle as O  # noqa: E402
from oracle import torch_kernels as T  # noqa: E402
from test_gpu_parity import _close, _grad_close  # noqa: E402

gpu = pytest.mark.gpu

WIDTHS = [1, 2, 3, 5, 8, 13, 16, 17, 31, 32]
ROW_NAMES = ['rbf', 'mix_rq_1dot', 'tanh_mix_rq', 'distance', 'dot']
STRIDE_NAMES = ['rbf', 'mix_rq_1dot', 'tanh_mix_rq', 'dot']
CAP = 8192                     # wave_grid: 2048 blocks x 4 waves, one row each

PARAM_KW = {
    'mix_rbf': dict(sigmas=(0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 13.0),
                    wts=(0.5, 1.5, 0.25, 2.0, 1.0, 0.75, 1.25, 3.0)),
    'mix_rq': dict(alphas=(0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0),
                   wts=(2.0, 0.5, 1.5, 0.25, 1.0, 3.0, 0.75, 1.25), add_dot=0.3),
}


def _cid(tag, name, shape, d):
    return '%s-%s-%s-d%d' % (tag, name, 'x'.join(str(s) for s in shape), d)


def _wit_cases():
    out = []
    for d in WIDTHS:
        out += [('width', n, (5, 70, 9), d) for n in O.KERNEL_NAMES]
    for shape in [(1, 1, 1), (64, 64, 64), (3, 130, 65), (70, 3, 129)]:
        out += [('rows', n, shape, d) for n in ROW_NAMES for d in (2, 16)]
    for shape in [(8200, 3, 2), (3, 8200, 5), (3, 5, 8200)]:
        out += [('stride', n, shape, 1) for n in STRIDE_NAMES]
    out += [('params', n, (5, 70, 9), 16) for n in PARAM_KW]
    return out


def _km_cases():
    out = []
    for d in WIDTHS:
        out += [('width', n, (19, 70), d) for n in O.KERNEL_NAMES]
    for shape in [(1, 1), (4, 64), (5, 65), (130, 3)]:
        out += [('rows', n, shape, d) for n in ROW_NAMES for d in (2, 16)]
    for shape in [(8200, 3), (3, 8200)]:
        out += [('stride', n, shape, 1) for n in STRIDE_NAMES]
    out += [('same', n, (33, 33), 5) for n in ROW_NAMES]      # K(A, A): one tensor, both sides
    out += [('params', n, (19, 70), 16) for n in PARAM_KW]
    return out


# a case whose first seed was ill-conditioned (module docstring) and the seed offset that is not
SEED_BUMP = {'wit-width-tanh_distance-5x70x9-d1': 8}
# ill-conditioned at each of 40 seeds: listed, counted by test_conditioning_caps, not run
DROPPED = frozenset(['wit-width-distance-5x70x9-d1'])

WIT_ALL, KM_ALL = _wit_cases(), _km_cases()
WIT_CASES = [c for c in WIT_ALL if 'wit-' + _cid(*c) not in DROPPED]
KM_CASES = [c for c in KM_ALL if 'km-' + _cid(*c) not in DROPPED]


def _spec_kw(case):
    return PARAM_KW[case[1]] if case[0] == 'params' else {}


MIN_SEP = 0.02


def _apart(rng, draw, n, others, tanh):
    """n seeded rows, each redrawn until it is at least MIN_SEP (as the kernel
    sees it: after tanh for the tanh kernels) from every row of ``others``.
    At a coincident pair the clamp of the Gram expansion, max(raw, 0), has a
    kink: whether fp32 rounds raw above or below 0 there switches an O(1)
    second-order term on or off, and 8200 x 3 points on a line always hold
    such a pair."""
    see = np.tanh if tanh else (lambda x: x)
    Z = draw(n)
    while True:
        close = np.zeros(n, bool)
        for o in others:
            dist2 = ((see(Z)[:, None, :] - see(o)[None, :, :]) ** 2).sum(-1)
            close |= (dist2 < MIN_SEP ** 2).any(1)
        if not close.any():
            return Z
        Z[close] = draw(int(close.sum()))


def _inputs(op, case):
    tag, name, shape, d = case
    key = op + '-' + _cid(*case)
    rng = np.random.default_rng((zlib.crc32(key.encode()) & 0xffff) + SEED_BUMP.get(key, 0))
    s = 1.0 / np.sqrt(d)
    tanh = name.startswith('tanh')

    def draw(shift):
        return lambda n: ((rng.standard_normal((n, d)) + shift) * s).astype(np.float32)
    if op == 'wit':
        b, nr, nf = shape
        if nr + nf > b:            # redraw on the long side
            H = draw(0.0)(b)
            R = _apart(rng, draw(0.0), nr, [H], tanh)
            F = _apart(rng, draw(0.5), nf, [H], tanh)
        else:
            R, F = draw(0.0)(nr), draw(0.5)(nf)
            H = _apart(rng, draw(0.0), b, [R, F], tanh)
        g = rng.standard_normal((b, d)).astype(np.float32)
        return H, R, F, g
    na, nb = shape
    if tag == 'same':
        A = draw(0.0)(na)
        return A, A, rng.standard_normal((na, nb)).astype(np.float32)
    if nb >= na:
        A = draw(0.0)(na)
        B = _apart(rng, draw(0.3), nb, [A], tanh)
    else:
        B = draw(0.3)(nb)
        A = _apart(rng, draw(0.0), na, [B], tanh)
    G = rng.standard_normal((na, nb)).astype(np.float32)
    return A, B, G


def _grads(loss, ts):
    gs = torch.autograd.grad(loss, ts, allow_unused=True)
    return [np.zeros(tuple(t.shape)) if g is None else g.numpy() for g, t in zip(gs, ts)]


def _wit_ref(spec, H, R, F, g, raw32):
    """(w, dH, gH, gR, gF) in float64 by autograd."""
    ts = [torch.tensor(a.astype(np.float64), requires_grad=True) for a in (H, R, F)]
    w = T.witness(spec, *ts, raw32=raw32).detach().numpy()
    dH = T.witness_grad_H(spec, *ts, create_graph=True, raw32=raw32)
    if dH.requires_grad:
        second = _grads((dH * torch.tensor(g.astype(np.float64))).sum(), ts)
    else:
        second = [np.zeros(tuple(t.shape)) for t in ts]
    return [w, dH.detach().numpy()] + second


def _km_ref(spec, A, B, G, raw32, same=False):
    """(K, gA, gB) in float64 by autograd; ``same``: K(A, A), gA is the sum."""
    At = torch.tensor(A.astype(np.float64), requires_grad=True)
    Bt = At if same else torch.tensor(B.astype(np.float64), requires_grad=True)
    K = T.kernel_xy(spec, At, Bt, raw32=raw32)
    loss = (K * torch.tensor(G.astype(np.float64))).sum()
    gs = _grads(loss, [At] if same else [At, Bt])
    return [K.detach().numpy()] + gs


def _bounds(op, ref, same=False):
    """Elementwise bound per checked quantity (module docstring)."""
    def first(r):
        return 1e-4 * max(np.abs(r).max(), 1e-12) + 1e-3 * np.abs(r)

    def second(r):
        return 2e-3 * np.abs(r).max() + 2e-3 * np.abs(r)
    value = 1e-5 + 1e-4 * np.abs(ref[0])
    if op == 'wit':
        return [value, first(ref[1])] + [second(r) for r in ref[2:]]
    return [value] + [first(r) for r in ref[1:]]


_REFS = {}


def _reference(op, case):
    """(inputs, plain reference, well-conditioned?) -- computed once per case
    and left unchanged."""
    key = op + '-' + _cid(*case)
    if key not in _REFS:
        spec = O.kernel_spec(case[1], **_spec_kw(case))
        inp = _inputs(op, case)
        if op == 'wit':
            plain, r32 = _wit_ref(spec, *inp, False), _wit_ref(spec, *inp, True)
        else:
            same = case[0] == 'same'
            plain, r32 = _km_ref(spec, *inp, False, same), _km_ref(spec, *inp, True, same)
        ok = all((np.abs(p - q) <= 0.25 * lim).all()
                 for p, q, lim in zip(plain, r32, _bounds(op, plain)))
        _REFS[key] = (inp, plain, ok)
    return _REFS[key]


def test_conditioning_caps():
    """From the reference alone: which cases the fp32 Gram expansion makes
    ill-posed.  None of the rbf / rq / dot kinds, at most 1 in 10 of the
    distance kinds, and exactly the ones listed in DROPPED."""
    bad, total, dropped = {}, {}, set()
    for op, cases in (('wit', WIT_ALL), ('km', KM_ALL)):
        for case in cases:
            kind = O.kernel_spec(case[1]).kind
            total[kind] = total.get(kind, 0) + 1
            if not _reference(op, case)[2]:
                bad[kind] = bad.get(kind, 0) + 1
                dropped.add(op + '-' + _cid(*case))
    print('ill-conditioned:', sorted(dropped), 'per kind:', bad, 'of', total)
    assert dropped == set(DROPPED)
    for kind in ('rbf', 'rq', 'dot'):
        assert bad.get(kind, 0) == 0
    assert bad.get('distance', 0) * 10 <= total['distance']


def _report(kind, order, got, ref, lim):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.max() > 0 else 0.0
    print('worst kind=%s order=%s err/bound=%.2e max err %.3e max|ref| %.3e' % (
        kind, order, ratio, err.max(), np.abs(ref).max()))


def _second_close(got, ref, what):
    _close(got, ref, 2e-3 * np.abs(ref).max(), 2e-3, what)


def _dev_tensors(dev, arrays, grad=True):
    return [torch.tensor(a, device=dev, requires_grad=grad) for a in arrays]


def _run_witness(dev, name, H, R, F, g, **kw):
    from gan.core import mmd
    ts = _dev_tensors(dev, (H, R, F))
    dH, w = mmd.witness_and_grad(*ts, kernel=name, **kw)
    (dH * torch.tensor(g, device=dev)).sum().backward()
    return [w.cpu().numpy(), dH.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in ts]


def _split(shape_rows):
    """Row ranges to check by name: below and from the grid cap."""
    if shape_rows > CAP:
        return [('rows < %d' % CAP, slice(0, CAP)), ('rows >= %d' % CAP, slice(CAP, None))]
    return [('all rows', slice(None))]


@gpu
@pytest.mark.parametrize('case', WIT_CASES, ids=lambda c: _cid(*c))
def test_witness(dev, case):
    tag, name, (b, nr, nf), d = case
    (H, R, F, g), ref, ok = _reference('wit', case)
    assert ok
    got = _run_witness(dev, name, H, R, F, g, **_spec_kw(case))
    kind = O.kernel_spec(name).kind
    lims = _bounds('wit', ref)
    for i, order in enumerate(('value', 'first', 'second', 'second', 'second')):
        _report(kind, order, got[i], ref[i], lims[i])
    for label, rows in _split(b):
        _close(got[0][rows], ref[0][rows], 1e-5, 1e-4, 'w, ' + label)
    # the gradient bounds take max|ref| over the whole tensor, so they are
    # checked whole; the failure message names the side of the cap
    for i, what in enumerate(('dH', 'gH', 'gR', 'gF'), start=1):
        err = np.abs(got[i] - ref[i])
        worst = int(np.unravel_index(np.argmax(err - lims[i]), err.shape)[0])
        what = '%s (worst row %d, %s %d)' % (what, worst, '>=' if worst >= CAP else '<', CAP)
        if i == 1:
            _grad_close(got[i], ref[i], what)
        else:
            _second_close(got[i], ref[i], what)


def _run_kmat(dev, name, A, B, G, need, same=False, **kw):
    from gan.core import mmd
    At = torch.tensor(A, device=dev, requires_grad=need[0])
    Bt = At if same else torch.tensor(B, device=dev, requires_grad=need[1])
    K = mmd.kernel_matrix(At, Bt, name, **kw)
    (K * torch.tensor(G, device=dev)).sum().backward()
    return (K.detach().cpu().numpy(), None if At.grad is None else At.grad.cpu().numpy(),
            None if Bt.grad is None else Bt.grad.cpu().numpy())


@gpu
@pytest.mark.parametrize('case', KM_CASES, ids=lambda c: _cid(*c))
def test_kernel_matrix(dev, case):
    tag, name, (na, nb), d = case
    (A, B, G), ref, ok = _reference('km', case)
    assert ok
    kind = O.kernel_spec(name).kind
    kw = _spec_kw(case)
    if tag == 'same':
        K, gA, _ = _run_kmat(dev, name, A, B, G, (True, True), same=True, **kw)
        _close(K, ref[0], 1e-5, 1e-4, 'K(A, A)')
        _grad_close(gA, ref[1], 'gA + gB of K(A, A)')
        return
    lims = _bounds('km', ref)
    for need in ((True, False), (False, True), (True, True)):
        K, gA, gB = _run_kmat(dev, name, A, B, G, need, **kw)
        for label, rows in _split(na):
            _close(K[rows], ref[0][rows], 1e-5, 1e-4, 'K, ' + label)
        assert (gA is not None) == need[0] and (gB is not None) == need[1]
        for i, (what, got) in enumerate((('gA', gA), ('gB', gB)), start=1):
            if got is None:
                continue
            err = np.abs(got - ref[i])
            worst = int(np.unravel_index(np.argmax(err - lims[i]), err.shape)[0])
            _grad_close(got, ref[i], '%s need=%s (worst row %d, %s %d)' % (
                what, need, worst, '>=' if worst >= CAP else '<', CAP))
    _report(kind, 'value', K, ref[0], lims[0])
    _report(kind, 'first', gA, ref[1], lims[1])
    _report(kind, 'first', gB, ref[2], lims[2])


# ---------------------------------------------------------------------------
# parameters: the term limit
# ---------------------------------------------------------------------------
def test_nine_terms_raise_before_any_launch():
    """More than SMMD_MAX_TERMS terms: a ValueError naming the limit out of
    KernelSpec.desc, i.e. while the arguments of the library call are built."""
    from gan.core import mmd
    spec = mmd.get_kernel_spec('mix_rbf', sigmas=tuple(float(i + 1) for i in range(9)))
    with pytest.raises(ValueError, match='SMMD_MAX_TERMS'):
        spec.desc()
    spec = mmd.get_kernel_spec('mix_rq', alphas=tuple(float(i + 1) for i in range(9)))
    with pytest.raises(ValueError, match='SMMD_MAX_TERMS'):
        spec.desc()
    assert mmd.get_kernel_spec('mix_rbf', sigmas=tuple(float(i + 1) for i in range(8))).desc() \
        .n_terms == 8


SENTINEL = -777.25


def _abi_witness_fwd(dev, desc, H, R, F, w, dH):
    from gan.core import _lib
    return _lib.lib().smmd_witness_fwd(
        desc, _lib.ptr(H), H.shape[0], _lib.ptr(R), R.shape[0], _lib.ptr(F), F.shape[0],
        H.shape[1], _lib.ptr(w), _lib.ptr(dH), _lib.stream_handle(dev))


@gpu
def test_nine_terms_write_nothing(dev):
    from gan.core import _lib, mmd
    H, R, F, g = _inputs('wit', ('width', 'mix_rbf', (5, 70, 9), 16))
    Ht, Rt, Ft = _dev_tensors(dev, (H, R, F), grad=False)
    nine = tuple(float(i + 1) for i in range(9))
    with pytest.raises(ValueError, match='SMMD_MAX_TERMS'):
        mmd.witness_and_grad(Ht, Rt, Ft, kernel='mix_rbf', sigmas=nine)
    with pytest.raises(ValueError, match='SMMD_MAX_TERMS'):
        mmd.kernel_matrix(Ht, Rt, 'mix_rq', alphas=nine)
    # the library's own guard, for a caller that fills the descriptor itself
    desc = mmd.get_kernel_spec('mix_rbf').desc()
    desc.n_terms = 9
    w = torch.full((5,), SENTINEL, device=dev)
    dH = torch.full((5, 16), SENTINEL, device=dev)
    st = _abi_witness_fwd(dev, desc, Ht, Rt, Ft, w, dH)
    torch.cuda.synchronize()
    assert st != 0 and b'SMMD_EINVAL' in _lib.lib().smmd_status_string(st)
    assert bool((w == SENTINEL).all()) and bool((dH == SENTINEL).all())


# ---------------------------------------------------------------------------
# width 33: no instantiation; pinned as an error that writes nothing
# ---------------------------------------------------------------------------
@gpu
def test_width_33_unsupported(dev):
    from gan.core import _lib, mmd
    rng = np.random.default_rng(33)
    H, R, F = (torch.tensor(rng.standard_normal((n, 33)).astype(np.float32), device=dev)
               for n in (5, 7, 9))
    with pytest.raises(_lib.SmmdError, match='SMMD_EUNSUPPORTED'):
        mmd.witness_and_grad(H, R, F, kernel='rbf')
    with pytest.raises(_lib.SmmdError, match='SMMD_EUNSUPPORTED'):
        mmd.kernel_matrix(H, R, 'rbf')
    L = _lib.lib()
    s = _lib.stream_handle(dev)
    desc = mmd.get_kernel_spec('rbf').desc()
    outs = {k: torch.full(shape, SENTINEL, device=dev) for k, shape in dict(
        w=(5,), dH=(5, 33), gH=(5, 33), gR=(7, 33), gF=(9, 33), K=(5, 7), gA=(5, 33),
        gB=(7, 33)).items()}
    G = torch.ones(5, 7, device=dev)
    p = _lib.ptr
    sts = [
        _abi_witness_fwd(dev, desc, H, R, F, outs['w'], outs['dH']),
        L.smmd_witness_bwd(desc, p(H), 5, p(R), 7, p(F), 9, 33, p(H), p(outs['gH']),
                           p(outs['gR']), p(outs['gF']), s),
        L.smmd_kernel_matrix_fwd(desc, p(H), 5, p(R), 7, 33, p(outs['K']), s),
        L.smmd_kernel_matrix_bwd(desc, p(H), 5, p(R), 7, 33, p(G), p(outs['gA']),
                                 p(outs['gB']), s),
    ]
    torch.cuda.synchronize()
    assert sts == [_lib.SMMD_EUNSUPPORTED] * 4
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), k


# ---------------------------------------------------------------------------
# fixed order, optional outputs, strides
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', O.KERNEL_NAMES)
def test_same_bits_twice(dev, name):
    """The header promises a fixed summation order: two runs, the same bits
    (lane stride, more than one block, ragged width)."""
    H, R, F, g = _inputs('wit', ('bits', name, (70, 130, 65), 5))
    a = _run_witness(dev, name, H, R, F, g)
    b = _run_witness(dev, name, H, R, F, g)
    for x, y, what in zip(a, b, ('w', 'dH', 'gH', 'gR', 'gF')):
        assert np.array_equal(x, y), what
    A, B, G = _inputs('km', ('bits', name, (70, 130), 5))
    a = _run_kmat(dev, name, A, B, G, (True, True))
    b = _run_kmat(dev, name, A, B, G, (True, True))
    for x, y, what in zip(a, b, ('K', 'gA', 'gB')):
        assert np.array_equal(x, y), what


@gpu
@pytest.mark.parametrize('name', ['rbf', 'tanh_distance'])
def test_optional_outputs_through_the_abi(dev, name):
    """out_w alone (out_dH NULL) and out_dH alone give the bits of the full call."""
    from gan.core import mmd
    H, R, F, g = _inputs('wit', ('abi', name, (70, 130, 65), 5))
    Ht, Rt, Ft = _dev_tensors(dev, (H, R, F), grad=False)
    desc = mmd.get_kernel_spec(name).desc()

    def call(want_w, want_dH):
        w = torch.full((70,), SENTINEL, device=dev) if want_w else None
        dH = torch.full((70, 5), SENTINEL, device=dev) if want_dH else None
        assert _abi_witness_fwd(dev, desc, Ht, Rt, Ft, w, dH) == 0
        torch.cuda.synchronize()
        return w, dH
    w, dH = call(True, True)
    assert bool((w != SENTINEL).all()) and bool((dH != SENTINEL).all())
    w1, none = call(True, False)
    none2, dH1 = call(False, True)
    assert none is None and none2 is None
    assert torch.equal(w1, w) and torch.equal(dH1, dH)


@gpu
@pytest.mark.parametrize('name', ['mix_rq_1dot', 'tanh_distance'])
def test_non_contiguous_inputs(dev, name):
    """Strided H / R / F and a strided incoming gradient give the bits of
    their contiguous copies."""
    from gan.core import mmd
    rng = np.random.default_rng(9)
    b, nr, nf, d = 70, 130, 65, 5
    wide = [torch.tensor((rng.standard_normal((n, 2 * d)) * 0.5).astype(np.float32), device=dev)
            for n in (b, nr, nf)]
    gT = torch.tensor(rng.standard_normal((d, b)).astype(np.float32), device=dev)
    outs = []
    for contiguous in (False, True):
        ts = [t[:, ::2] for t in wide]
        gd = gT.t()
        assert not ts[0].is_contiguous() and not gd.is_contiguous()
        if contiguous:
            ts, gd = [t.contiguous() for t in ts], gd.contiguous()
        ts = [t.detach().requires_grad_(True) for t in ts]
        dH, w = mmd.witness_and_grad(*ts, kernel=name)
        dH.backward(gd)
        outs.append([w, dH.detach()] + [t.grad for t in ts])
    for x, y, what in zip(outs[0], outs[1], ('w', 'dH', 'gH', 'gR', 'gF')):
        assert torch.equal(x, y), what
    # the kernel matrix: strided A, B and a strided G
    GT = torch.tensor(rng.standard_normal((nr, b)).astype(np.float32), device=dev)
    outs = []
    for contiguous in (False, True):
        A, B, G = wide[0][:, ::2], wide[1][:, ::2], GT.t()
        if contiguous:
            A, B, G = A.contiguous(), B.contiguous(), G.contiguous()
        A, B = A.detach().requires_grad_(True), B.detach().requires_grad_(True)
        K = mmd.kernel_matrix(A, B, name)
        K.backward(G)
        outs.append([K.detach(), A.grad, B.grad])
    for x, y, what in zip(outs[0], outs[1], ('K', 'gA', 'gB')):
        assert torch.equal(x, y), what
