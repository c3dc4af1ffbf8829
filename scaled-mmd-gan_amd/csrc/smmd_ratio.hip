// smmd_ratio.hip -- the variance-normalised MMD objective: MMD^2, its variance
// estimate and the t-statistic mmd2 / sqrt(max(var_est, min_var_est)), with
// the two unit gradients d mmd2 / dZ and d var_est / dZ, Z = [X; Y].
//
// Reference: gan/core/mmd.py:223-293 (mmd2_and_ratio, _mmd2_and_ratio,
// _mmd2_and_variance) and TF's autodiff of them, on the kernel family of
// mmd.py:18-188.  The reference's values are kept term for term, its quirks
// included: the "unbiased" mmd2 keeps the diagonal sums in its numerators
// (:274-276), and a kernel with a constant diagonal subtracts that constant
// where the matrix holds the computed diagonal (:241-257), so for the
// mix_rq_*dot kernels e_i = K_ii - const stays in the row sums.
//
// No N x N array is written.  One forward call is a short chain of launches:
//
//   prep      Z (tanh applied when the kernel asks) into a side-padded copy
//             Zp [2 mp][dp], mp = m rounded up to 64: every 64-row tile is all
//             X or all Y; ||z||^2 per row; the MFMA path also keeps Zp^T
//   sweep 1   every ordered pair once: per row and per column chunk the sums
//             of K and K^2 over the same-side columns (diagonal excluded) and
//             over the other side's, fp32 inside a chunk
//   rowsum    the chunks summed in chunk order, in double
//   final     one block: the scalar sums from the row statistics (double,
//             fixed order), mmd2, var_est, ratio, and per row the two
//             coefficients s_same / s_cross of the gradient's pair weights
//   sweep 2   (gradient requested) K and (al, be) recomputed per pair; the
//             pair's weight in d var_est is affine in K and the two rows'
//             coefficients:  w = P0 + P1 K + s[row] + s[col]  (same-side pairs
//             use s_same and the side's P0, cross pairs s_cross); per row and
//             chunk  g = z_i sum_j w (al + be) - sum_j (w be) z_j  for both
//             weightings (mmd2's w is a constant per side pairing)
//   gradsum   the chunks summed in chunk order in double, the diagonal's term
//             (2 al_ii z_i times d / dK_ii) and the tanh factor
//   clear     the workspace back to zero
//
// Two sweeps' kernels, chosen by d:
//  * d <= 8, after smmd_mmd_tile.hip: a lane owns a row, a wave walks its run
//    of columns with the column's features (and its coefficient) in SGPRs,
//    grid = row tiles x column chunks, the 4 waves' partials summed in LDS in
//    wave order.
//  * d > 8, v_mfma_f32_32x32x2_f32: a block of 4 waves (2 x 2, 32 x 32 pairs
//    each) takes 64-row x 64-column pair tiles, a run of `tpc` column tiles
//    of one side per block.  The Gram block comes from MFMAs over dp (d zero-
//    padded to 4); both operands are read as fragments straight from Zp^T
//    (32 consecutive rows per half wave: coalesced), so the K loop has no LDS
//    staging and no barrier.  The kernel evaluation runs on the accumulators.
//    Sweep 1 keeps a lane's 16 row partials in registers over the run and
//    folds the 32 columns by a fixed butterfly at the end.  Sweep 2 writes the
//    two weight tiles w be to LDS PT[2][64][65] (stride 65: a fragment read
//    walks 32 rows on 32 banks) and uses them as the A operand of a second
//    MFMA against the column rows of Zp (B fragments: 32 consecutive features
//    of one row, from global memory), 64 features per accumulator, NF = 1 or
//    2 accumulators per weighting; grid.z covers wider d.
//
// Every sum has a fixed order: no atomics and no arrival tickets anywhere.
#include "smmd_common.hpp"
#include "smmd_kern.hpp"
#include "smmd_pair.hpp"

#include <stdlib.h>

namespace smmd {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int RT = 64;                 // rows of a tile, columns of a pair tile
constexpr int R_WAVES = 4;
constexpr int R_TARGET_BLOCKS = 512;   // tile path: as smmd_mmd_tile.hip
constexpr int R_MIN_CPW = 32;
constexpr int R_MFMA_BLOCKS = 256;     // MFMA path: blocks aimed at before chunks stop splitting

// pair-weight scalars written by the final kernel (floats)
enum { SC_P0X, SC_P0Y, SC_P0C, SC_P1S, SC_P1C, SC_WMS, SC_WMC, SC_N = 8 };

struct RatioArgs {
    const float *X, *Y;
    int m, d, dp, mp, Rp;
    int kind, tanh_in, has_const, biased, mfma;
    double const_diag, min_var;
    KParams kp;
    // workspace
    float *Zp, *ZpT, *sq;
    float *part1;       // [n_cc][4][Rp]: sum K same, sum K cross, sum K^2 same, sum K^2 cross
    double *rowstat;    // [4][Rp]
    float4 *coef;       // [Rp]: s_same, s_cross, diagonal coefficient of d mmd2, of d var_est
    float *scal;        // [SC_N]
    float *part2;       // [n_cc][2][Rp][dp]
    int n_cc;           // column chunks
    int cpw;            // tile path: columns per wave
    int nts, ncs, tpc, nfg;   // MFMA path: tiles per side, chunks per side, tiles per chunk
    float *out;
    float *gm_x, *gm_y, *gv_x, *gv_y;
};

// ---------------------------------------------------------------------------
// prep: one wave per padded row
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ratio_prep_kernel(RatioArgs a) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.Rp) return;
    const int side = p >= a.mp, loc = p - side * a.mp;
    const float *src = (loc < a.m) ? (side ? a.Y : a.X) + (size_t)loc * a.d : nullptr;
    float s = 0.f;
    for (int k = lane; k < a.dp; k += 64) {
        float v = 0.f;
        if (src && k < a.d) {
            v = src[k];
            if (a.tanh_in) v = tanhf(v);
        }
        a.Zp[(size_t)p * a.dp + k] = v;
        if (a.mfma) a.ZpT[(size_t)k * a.Rp + p] = v;
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) a.sq[p] = s;
}

// ---------------------------------------------------------------------------
// d <= 8: lane owns a row, column features in SGPRs
// ---------------------------------------------------------------------------
// Columns [j0, j1) of one side (S: that side's rows of Zp, dd floats each;
// A: that side's coefficient records, or unused).  The column index is
// wave-uniform, so these are scalar loads: 8 columns per batch, the next
// batch's loads issued before this batch is evaluated.
template <int DT, bool AUX>
__device__ __forceinline__ void rload(const float *__restrict__ S, const float *__restrict__ A,
                                      int dd, int j, float (&zb)[8][DT], float (&ab)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
        for (int k = 0; k < DT; ++k) zb[u][k] = (k < dd) ? S[(size_t)(j + u) * dd + k] : 0.f;
        ab[u] = AUX ? A[(size_t)(j + u) * 4] : 0.f;
    }
}

template <int DT, bool AUX, class F>
__device__ __forceinline__ void col_sweep(const float *__restrict__ S, const float *__restrict__ A,
                                          int d, int j0, int j1, F &&pair) {
    const int dd = (DT == 1) ? 1 : d;
    int j = j0;
    if (j + 8 <= j1) {
        float nb[8][DT], na[8];
        rload<DT, AUX>(S, A, dd, j, nb, na);
        for (; j + 8 <= j1; j += 8) {
            float cb[8][DT], ca[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
#pragma unroll
                for (int k = 0; k < DT; ++k) cb[u][k] = nb[u][k];
                ca[u] = na[u];
            }
            if (j + 16 <= j1) rload<DT, AUX>(S, A, dd, j + 8, nb, na);
#pragma unroll
            for (int u = 0; u < 8; ++u) pair(j + u, cb[u], ca[u]);
        }
    }
    for (; j < j1; ++j) {
        float zc[DT];
#pragma unroll
        for (int k = 0; k < DT; ++k) zc[k] = (k < dd) ? S[(size_t)j * dd + k] : 0.f;
        pair(j, zc, AUX ? A[(size_t)j * 4] : 0.f);
    }
}

// GRAD false: sweep 1 (row statistics); true: sweep 2 (the two unit gradients)
template <int DT, int KIND, int NT, bool GRAD>
__global__ __launch_bounds__(RT * R_WAVES) void ratio_tile_kernel(RatioArgs a) {
    constexpr int NV = GRAD ? 2 * (DT + 1) : 4;
    __shared__ float lds_v[R_WAVES][NV][RT];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ch = blockIdx.x % a.n_cc, rt = blockIdx.x / a.n_cc;
    const int p = rt * RT + lane;
    const int side = (rt * RT >= a.mp) ? 1 : 0;          // uniform: tiles never straddle
    const int loc = p - side * a.mp;
    const bool active = loc < a.m;
    PairEval<KIND, NT> pe;
    pe.init(a.kp);

    float zi[DT];
#pragma unroll
    for (int k = 0; k < DT; ++k) zi[k] = (k < a.d) ? a.Zp[(size_t)p * a.d + k] : 0.f;
    const float sqi = tdot<DT>(zi, zi);
    float srow_same = 0.f, srow_cross = 0.f;
    if (GRAD) {
        const float4 c = a.coef[p];
        srow_same = c.x;
        srow_cross = c.y;
    }

    float v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.f;

    // this wave's columns [c0, c1) of the column list [X (m); Y (m)]
    const int c0 = (ch * R_WAVES + w) * a.cpw;
    const int c1 = min(c0 + a.cpw, 2 * a.m);
    for (int cs = 0; cs < 2; ++cs) {                     // the run's X part, then its Y part
        const int j0 = max(c0, cs * a.m) - cs * a.m, j1 = min(c1, (cs + 1) * a.m) - cs * a.m;
        if (j0 >= j1) continue;
        const bool same = cs == side;
        const int selfj = same ? loc : -1;
        const float *S = a.Zp + (size_t)cs * a.mp * a.d;
        const float *A = reinterpret_cast<const float *>(a.coef + (size_t)cs * a.mp) + (same ? 0 : 1);
        float P0 = 0.f, P1 = 0.f, wm = 0.f;
        if (GRAD) {
            P0 = same ? a.scal[side ? SC_P0Y : SC_P0X] : a.scal[SC_P0C];
            P1 = a.scal[same ? SC_P1S : SC_P1C];
            wm = a.scal[same ? SC_WMS : SC_WMC];
        }
        const float srow = same ? srow_same : srow_cross;
        float ks = 0.f, kq = 0.f;                        // sweep 1: this part's sums
        col_sweep<DT, GRAD>(S, A, a.d, j0, j1, [&](int j, const float (&zc)[DT], float scol) {
            const float sqc = tdot<DT>(zc, zc);
            const float dot = tdot<DT>(zi, zc);
            const float raw = (-2.f * dot + sqi) + sqc;      // mmd.py:67 order
            float K, al, be;
            pe.eval(a.kp, raw, dot, sqi, sqc, K, al, be);
            const bool self = j == selfj;
            if (!GRAD) {
                if (self) K = 0.f;
                ks += K;
                kq = fmaf(K, K, kq);
            } else {
                float wv = fmaf(P1, K, (P0 + srow) + scol);
                float wmm = wm;
                if (self) { wv = 0.f; wmm = 0.f; }
                v[DT] = fmaf(wmm, al, v[DT]);
                v[2 * DT + 1] = fmaf(wv, al, v[2 * DT + 1]);
                const float cm = wmm * be, cv = wv * be;
#pragma unroll
                for (int k = 0; k < DT; ++k) {
                    const float df = zi[k] - zc[k];
                    v[k] = fmaf(cm, df, v[k]);
                    v[DT + 1 + k] = fmaf(cv, df, v[DT + 1 + k]);
                }
            }
        });
        if (!GRAD) {                                     // (constant indices: v stays in registers)
            v[0] += same ? ks : 0.f;
            v[1] += same ? 0.f : ks;
            v[2] += same ? kq : 0.f;
            v[3] += same ? 0.f : kq;
        }
    }
    if (!active) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) lds_v[w][k][lane] = v[k];
    __syncthreads();
    if (w != 0) return;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        v[k] = ((lds_v[0][k][lane] + lds_v[1][k][lane]) + lds_v[2][k][lane]) + lds_v[3][k][lane];
    if (!GRAD) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.part1[((size_t)ch * 4 + k) * a.Rp + p] = v[k];
    } else {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int k = 0; k < DT; ++k)
                if (k < a.d)
                    a.part2[(((size_t)ch * 2 + s) * a.Rp + p) * a.d + k] =
                        fmaf(v[s * (DT + 1) + DT], zi[k], v[s * (DT + 1) + k]);
    }
}

// ---------------------------------------------------------------------------
// d > 8: 64 x 64 pair tiles on the f32 MFMA
// ---------------------------------------------------------------------------
// row of accumulator element r of a 32 x 32 MFMA tile (column: lane & 31)
__device__ __forceinline__ int mfma_row(int r, int lane) {
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// the wave's 32 x 32 block of Z_rows Z_cols^T over dp, fragments from Zp^T
__device__ __forceinline__ floatx16 gram_block(const RatioArgs &a, int prow, int pcol, int lane) {
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *ap = a.ZpT + (size_t)(lane >> 5) * a.Rp + prow + (lane & 31);
    const float *bp = a.ZpT + (size_t)(lane >> 5) * a.Rp + pcol + (lane & 31);
    const size_t step = 2 * (size_t)a.Rp;
    for (int k = 0; k < a.dp; k += 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(*ap, *bp, acc, 0, 0, 0);
        ap += step;
        bp += step;
    }
    return acc;
}

// fold a lane's 16 row partials over the 32 columns of its half wave
__device__ __forceinline__ void fold32(float (&x)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) x[r] += __shfl_xor(x[r], off, SMMD_WAVE);
}

template <int KIND, int NT>
__global__ __launch_bounds__(256) void ratio_mfma_s1_kernel(RatioArgs a) {
    __shared__ float rsq[RT];
    __shared__ float red[2][2][RT];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int cc = blockIdx.x, rt = blockIdx.y;
    const int side_c = cc / a.ncs, chunk = cc % a.ncs;
    const int side_r = rt >= a.nts;
    const bool same = side_c == side_r;
    const int p0 = rt * RT;
    if (threadIdx.x < RT) rsq[threadIdx.x] = a.sq[p0 + threadIdx.x];
    __syncthreads();
    PairEval<KIND, NT> pe;
    pe.init(a.kp);
    float rs[16], rq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rs[r] = rq[r] = 0.f;
    const int t1 = min((chunk + 1) * a.tpc, a.nts);
    for (int t = chunk * a.tpc; t < t1; ++t) {
        const int jp0 = side_c * a.mp + t * RT;
        const int jp = jp0 + wn * 32 + (lane & 31);
        const bool colvalid = jp - side_c * a.mp < a.m;
        const floatx16 acc = gram_block(a, p0 + wm * 32, jp0 + wn * 32, lane);
        const float sqc = a.sq[jp];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 32 + mfma_row(r, lane);
            const float sqi = rsq[rl], dot = acc[r];
            const float raw = (-2.f * dot + sqi) + sqc;          // mmd.py:67 order
            float K, al, be;
            pe.eval(a.kp, raw, dot, sqi, sqc, K, al, be);
            if (!colvalid || (same && p0 + rl == jp)) K = 0.f;
            rs[r] += K;
            rq[r] = fmaf(K, K, rq[r]);
        }
    }
    fold32(rs);
    fold32(rq);
    if ((lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 32 + mfma_row(r, lane);
            red[wn][0][rl] = rs[r];
            red[wn][1][rl] = rq[r];
        }
    }
    __syncthreads();
    if (threadIdx.x < RT) {
        const int t = threadIdx.x;
        const float s = red[0][0][t] + red[1][0][t], q = red[0][1][t] + red[1][1][t];
        float *dst = a.part1 + (size_t)cc * 4 * a.Rp + p0 + t;
        dst[0] = same ? s : 0.f;
        dst[(size_t)a.Rp] = same ? 0.f : s;
        dst[2 * (size_t)a.Rp] = same ? q : 0.f;
        dst[3 * (size_t)a.Rp] = same ? 0.f : q;
    }
}

template <int KIND, int NT, int NF>
__global__ __launch_bounds__(256) void ratio_mfma_s2_kernel(RatioArgs a) {
    __shared__ float rsq[RT], rss[RT];
    __shared__ float PT[2][RT][RT + 1];
    __shared__ float ured[2][2][RT];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int cc = blockIdx.x, rt = blockIdx.y, fg = blockIdx.z;
    const int side_c = cc / a.ncs, chunk = cc % a.ncs;
    const int side_r = rt >= a.nts;
    const bool same = side_c == side_r;
    const int p0 = rt * RT;
    if (threadIdx.x < RT) {
        rsq[threadIdx.x] = a.sq[p0 + threadIdx.x];
        const float4 c = a.coef[p0 + threadIdx.x];
        rss[threadIdx.x] = same ? c.x : c.y;
    }
    __syncthreads();
    const float P0 = same ? a.scal[side_r ? SC_P0Y : SC_P0X] : a.scal[SC_P0C];
    const float P1 = a.scal[same ? SC_P1S : SC_P1C];
    const float wm0 = a.scal[same ? SC_WMS : SC_WMC];
    PairEval<KIND, NT> pe;
    pe.init(a.kp);
    float um[16], uv[16];
    floatx16 g[2][NF];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        um[r] = uv[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < NF; ++c) g[s][c][r] = 0.f;
    }
    const int fbase = fg * NF * 64 + wn * 32 + (lane & 31);   // + 64 c: this lane's feature
    const int cl = wn * 32 + (lane & 31);
    const int t1 = min((chunk + 1) * a.tpc, a.nts);
    for (int t = chunk * a.tpc; t < t1; ++t) {
        const int jp0 = side_c * a.mp + t * RT;
        const int jp = jp0 + cl;
        const bool colvalid = jp - side_c * a.mp < a.m;
        const floatx16 acc = gram_block(a, p0 + wm * 32, jp0 + wn * 32, lane);
        const float sqc = a.sq[jp];
        const float4 ccoef = a.coef[jp];
        const float scol = same ? ccoef.x : ccoef.y;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 32 + mfma_row(r, lane);
            const float sqi = rsq[rl], dot = acc[r];
            const float raw = (-2.f * dot + sqi) + sqc;
            float K, al, be;
            pe.eval(a.kp, raw, dot, sqi, sqc, K, al, be);
            float wv = fmaf(P1, K, (P0 + rss[rl]) + scol);
            float wmm = wm0;
            if (!colvalid || (same && p0 + rl == jp)) { wv = 0.f; wmm = 0.f; }
            const float pm = wmm * be, pv = wv * be;
            um[r] += fmaf(wmm, al, pm);
            uv[r] += fmaf(wv, al, pv);
            PT[0][rl][cl] = pm;
            PT[1][rl][cl] = pv;
        }
        __syncthreads();
        // G += PT (64 x 64 j) x Zp[column rows] (64 j x 64 NF features)
        const float *a0 = &PT[0][wm * 32 + (lane & 31)][lane >> 5];
        const float *a1 = &PT[1][wm * 32 + (lane & 31)][lane >> 5];
        const float *zb = a.Zp + (size_t)(jp0 + (lane >> 5)) * a.dp;
#pragma unroll 4
        for (int kk = 0; kk < RT / 2; ++kk) {
            const float fa0 = a0[2 * kk], fa1 = a1[2 * kk];
#pragma unroll
            for (int c = 0; c < NF; ++c) {
                const int f = fbase + 64 * c;
                const float b = (f < a.dp) ? zb[(size_t)2 * kk * a.dp + f] : 0.f;
                g[0][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0, b, g[0][c], 0, 0, 0);
                g[1][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1, b, g[1][c], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    fold32(um);
    fold32(uv);
    if ((lane & 31) == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 32 + mfma_row(r, lane);
            ured[wn][0][rl] = um[r];
            ured[wn][1][rl] = uv[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NF; ++c) {
        const int f = fbase + 64 * c;
        if (f >= a.dp) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wm * 32 + mfma_row(r, lane);
            const size_t p = p0 + rl;
            const float z = a.Zp[p * a.dp + f];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float u = ured[0][s][rl] + ured[1][s][rl];
                a.part2[(((size_t)cc * 2 + s) * a.Rp + p) * a.dp + f] = fmaf(z, u, -g[s][c][r]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// the reductions between and after the sweeps
// ---------------------------------------------------------------------------
// sum of n floats `stride` apart, in index order, in double; 8 loads in flight
__device__ __forceinline__ double chunk_sum(const float *__restrict__ x, int n, size_t stride) {
    double s = 0.0;
    for (int c = 0; c < n; c += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = (c + u < n) ? x[(size_t)(c + u) * stride] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c + u < n) s += (double)t[u];
    }
    return s;
}

__global__ __launch_bounds__(256) void ratio_rowsum_kernel(RatioArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.Rp) return;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        a.rowstat[(size_t)k * a.Rp + p] =
            chunk_sum(a.part1 + (size_t)k * a.Rp + p, a.n_cc, 4 * (size_t)a.Rp);
}

// K(z, z) and al of the pair (i, i): raw D2 = 0, <z, z> = ||z||^2
__device__ __forceinline__ void diag_eval(const RatioArgs &a, float sq, float &K, float &al) {
    float be;
    switch (a.kind) {
        case SMMD_KIND_RBF: Kern<SMMD_KIND_RBF>::eval(a.kp, 0.f, sq, sq, sq, K, al, be); break;
        case SMMD_KIND_RQ: Kern<SMMD_KIND_RQ>::eval(a.kp, 0.f, sq, sq, sq, K, al, be); break;
        case SMMD_KIND_DISTANCE:
            Kern<SMMD_KIND_DISTANCE>::eval(a.kp, 0.f, sq, sq, sq, K, al, be);
            break;
        default: Kern<SMMD_KIND_DOT>::eval(a.kp, 0.f, sq, sq, sq, K, al, be); break;
    }
}

template <int NV>
__device__ __forceinline__ void block_sums_d(double (&v)[NV], double (*red)[NV]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[w][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// One block.  Per side: 0 sum Kt, 1 sum Kt^2, 2 sum r, 3 sum r^2, 4 <Kt, r>,
// 5 sum K^2 same-side off-diagonal, 6 sum K^2 cross, 7 sum diag, 8 sum diag2
// correction, with Kt_i = (row sum without the diagonal) + (K_ii - diag_i) and
// diag_i the constant or K_ii (mmd.py:241-257).
__global__ __launch_bounds__(256) void ratio_final_kernel(RatioArgs a) {
    __shared__ double red[4][18];
    double v[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) v[k] = 0.0;
    for (int p = threadIdx.x; p < a.Rp; p += 256) {
        const int side = p >= a.mp;
        if (p - side * a.mp >= a.m) continue;
        float Kd, al;
        diag_eval(a, a.sq[p], Kd, al);
        const double kd = Kd, dg = a.has_const ? a.const_diag : kd;
        const double kt = a.rowstat[p] + (kd - dg), r = a.rowstat[(size_t)a.Rp + p];
        const double t[9] = {kt, kt * kt, r, r * r, kt * r, a.rowstat[2 * (size_t)a.Rp + p],
                             a.rowstat[3 * (size_t)a.Rp + p], dg, kd * kd - dg * dg};
#pragma unroll
        for (int k = 0; k < 9; ++k) {       // (constant indices: v stays in registers)
            v[k] += side ? 0.0 : t[k];
            v[9 + k] += side ? t[k] : 0.0;
        }
    }
    block_sums_d<18>(v, red);
    const double m = a.m, m1 = m - 1.0;
    const double A = v[0], B = v[9], C = v[2];
    const double KtXX2 = v[5] + v[8], KtYY2 = v[14] + v[17], KXY2 = v[6];
    const double den = a.biased ? m * m : m * m1;
    const double mmd2 = (A + v[7]) / den + (B + v[16]) / den - 2.0 * C / (m * m);   // :269-276
    const double c1 = 2.0 / (m * m * m1 * m1);                                   // :279
    const double c2 = (4.0 * m - 6.0) / (m * m * m * m1 * m1 * m1);              // :282
    const double c3 = 4.0 * (m - 2.0) / (m * m * m * m1 * m1);                   // :283
    const double c4 = 4.0 * (m - 3.0) / (m * m * m * m1 * m1);                   // :285
    const double c5 = (8.0 * m - 12.0) / (m * m * m * m * m * m1);               // :286
    const double c6 = 8.0 / (m * m * m * m1);                                    // :287
    const double var = c1 * (2.0 * v[1] - KtXX2 + 2.0 * v[10] - KtYY2) - c2 * (A * A + B * B) +
                       c3 * (v[3] + v[12]) - c4 * KXY2 - c5 * C * C +
                       c6 * (1.0 / m * (A + B) * C - v[4] - v[13]);
    if (threadIdx.x == 0) {
        const bool clamped = !(var > a.min_var);
        const double vc = clamped ? a.min_var : var;
        a.out[0] = (float)mmd2;
        a.out[1] = (float)(mmd2 / sqrt(vc));
        a.out[2] = (float)var;
        a.out[3] = clamped ? 1.f : 0.f;
        a.out[4] = (float)vc;
        a.out[5] = a.out[6] = a.out[7] = 0.f;
        a.scal[SC_P0X] = (float)(-4.0 * c2 * A + 2.0 * c6 * C / m);
        a.scal[SC_P0Y] = (float)(-4.0 * c2 * B + 2.0 * c6 * C / m);
        a.scal[SC_P0C] = (float)(-2.0 * c5 * C + c6 * (A + B) / m);
        a.scal[SC_P1S] = (float)(-4.0 * c1);
        a.scal[SC_P1C] = (float)(-2.0 * c4);
        a.scal[SC_WMS] = (float)(2.0 / den);
        a.scal[SC_WMC] = (float)(-2.0 / (m * m));
        a.scal[7] = 0.f;
    }
    for (int p = threadIdx.x; p < a.Rp; p += 256) {
        const int side = p >= a.mp;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p - side * a.mp < a.m) {
            float Kd, al;
            diag_eval(a, a.sq[p], Kd, al);
            const double kd = Kd, dg = a.has_const ? a.const_diag : kd;
            const double kt = a.rowstat[p] + (kd - dg), r = a.rowstat[(size_t)a.Rp + p];
            c.x = (float)(4.0 * c1 * kt - c6 * r);
            c.y = (float)(2.0 * c3 * r - c6 * kt);
            // d / dK_ii, times dK_ii / dz_i = 2 al z_i.  A computed diagonal
            // cancels out of Kt and Kt^2 and enters only mmd2.
            c.z = (float)(2.0 * al / den);
            if (a.has_const)
                c.w = (float)(2.0 * al * (c1 * (4.0 * kt - 2.0 * kd) - 2.0 * c2 * (side ? B : A) +
                                          c6 * (C / m - r)));
        }
        a.coef[p] = c;
    }
}

// unit gradients: chunks in chunk order (double), the diagonal, the tanh factor
__global__ __launch_bounds__(256) void ratio_gradsum_kernel(RatioArgs a) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.Rp * a.dp) return;
    const int p = (int)(idx / a.dp), k = (int)(idx % a.dp);
    const int side = p >= a.mp, loc = p - side * a.mp;
    if (loc >= a.m || k >= a.d) return;
    const float z = a.Zp[idx];
    const float4 c = a.coef[p];
    const size_t cstride = 2 * (size_t)a.Rp * a.dp;
    double gm = chunk_sum(a.part2 + idx, a.n_cc, cstride);
    double gv = chunk_sum(a.part2 + (size_t)a.Rp * a.dp + idx, a.n_cc, cstride);
    gm += (double)c.z * z;
    gv += (double)c.w * z;
    if (a.tanh_in) {
        const double t = 1.0 - (double)z * z;
        gm *= t;
        gv *= t;
    }
    const size_t o = (size_t)loc * a.d + k;
    (side ? a.gm_y : a.gm_x)[o] = (float)gm;
    (side ? a.gv_y : a.gv_x)[o] = (float)gv;
}

__global__ __launch_bounds__(256) void ratio_clear_kernel(uint4 *p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct RatioBwdArgs {
    const float *out, *g_mmd2, *g_ratio, *g_var;
    const float *gm_x, *gm_y, *gv_x, *gv_y;
    float *dX, *dY;
    size_t n;             // m * d
};

__global__ __launch_bounds__(256) void ratio_bwd_kernel(RatioBwdArgs b) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * b.n) return;
    const double gm = b.g_mmd2 ? b.g_mmd2[0] : 0.0, gr = b.g_ratio ? b.g_ratio[0] : 0.0;
    const double gv = b.g_var ? b.g_var[0] : 0.0;
    const double mmd2 = b.out[0], v = b.out[4];
    const bool clamped = b.out[3] != 0.f;
    const float ca = (float)(gm + gr / sqrt(v));
    const float cb = (float)(gv - (clamped ? 0.0 : 0.5 * gr * mmd2 / (v * sqrt(v))));
    if (i < b.n) b.dX[i] = fmaf(ca, b.gm_x[i], cb * b.gv_x[i]);
    else b.dY[i - b.n] = fmaf(ca, b.gm_y[i - b.n], cb * b.gv_y[i - b.n]);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int renv_int(const char *k, int dflt) {
    const char *e = getenv(k);
    return (e && e[0]) ? atoi(e) : dflt;
}

static int tile_dt_of(int d) { return d <= 1 ? 1 : d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : 0; }

// Geometry and workspace layout of one (m, d); `a` gets the sizes, and the
// pointers when ws is given.  Returns the bytes used.
static size_t ratio_plan(int m, int d, RatioArgs &a, char *ws) {
    a.m = m;
    a.d = d;
    a.mfma = tile_dt_of(d) == 0;
    a.dp = a.mfma ? (d + 3) / 4 * 4 : d;
    a.mp = (m + RT - 1) / RT * RT;
    a.Rp = 2 * a.mp;
    a.nts = a.mp / RT;
    const int n_rt = 2 * a.nts;
    if (a.mfma) {
        // a run of tpc column tiles of one side per block: chunks split while
        // the grid stays under R_MFMA_BLOCKS (SMMD_RATIO_CHUNKS caps the
        // chunks per side: tuning, and the tests' tpc > 1 case)
        a.nfg = (a.dp + 127) / 128;
        if (a.dp <= 64) a.nfg = 1;
        int ncs = (R_MFMA_BLOCKS + n_rt * a.nfg - 1) / (n_rt * a.nfg);
        const int cap = renv_int("SMMD_RATIO_CHUNKS", 0);
        if (cap > 0 && ncs > cap) ncs = cap;
        if (ncs > a.nts) ncs = a.nts;
        if (ncs < 1) ncs = 1;
        a.tpc = (a.nts + ncs - 1) / ncs;
        a.ncs = (a.nts + a.tpc - 1) / a.tpc;
        a.n_cc = 2 * a.ncs;
        a.cpw = 0;
    } else {
        const int cols = 2 * m;
        const int max_ch = (cols + R_WAVES * R_MIN_CPW - 1) / (R_WAVES * R_MIN_CPW);
        int ch = (R_TARGET_BLOCKS + n_rt - 1) / n_rt;
        if (ch > max_ch) ch = max_ch;
        if (ch < 1) ch = 1;
        int cpw = (cols + R_WAVES * ch - 1) / (R_WAVES * ch);
        cpw = (cpw + 7) / 8 * 8;                    // whole 8-column batches
        a.cpw = cpw;
        a.n_cc = (cols + R_WAVES * cpw - 1) / (R_WAVES * cpw);
        a.nfg = a.ncs = a.tpc = 0;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = ws ? ws + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    const size_t Rp = a.Rp, dp = a.dp;
    a.Zp = (float *)take(Rp * dp * 4);
    a.ZpT = (float *)take(a.mfma ? Rp * dp * 4 : 0);
    a.sq = (float *)take(Rp * 4);
    a.part1 = (float *)take((size_t)a.n_cc * 4 * Rp * 4);
    a.rowstat = (double *)take(4 * Rp * 8);
    a.coef = (float4 *)take(Rp * 16);
    a.scal = (float *)take(SC_N * 4);
    a.part2 = (float *)take((size_t)a.n_cc * 2 * Rp * dp * 4);
    return off;
}

template <int DT, int KIND, int NT>
static void launch_ratio_tile(const RatioArgs &a, bool grad, hipStream_t s) {
    const dim3 grid(2 * a.nts * a.n_cc), block(RT * R_WAVES);
    if (grad) hipLaunchKernelGGL((ratio_tile_kernel<DT, KIND, NT, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ratio_tile_kernel<DT, KIND, NT, false>), grid, block, 0, s, a);
}

template <int KIND, int NT>
static void launch_ratio_sweep(const RatioArgs &a, bool grad, hipStream_t s) {
    if (a.mfma) {
        const dim3 block(256);
        if (!grad)
            hipLaunchKernelGGL((ratio_mfma_s1_kernel<KIND, NT>), dim3(a.n_cc, 2 * a.nts), block, 0,
                               s, a);
        else if (a.dp <= 64)
            hipLaunchKernelGGL((ratio_mfma_s2_kernel<KIND, NT, 1>), dim3(a.n_cc, 2 * a.nts, 1),
                               block, 0, s, a);
        else
            hipLaunchKernelGGL((ratio_mfma_s2_kernel<KIND, NT, 2>),
                               dim3(a.n_cc, 2 * a.nts, a.nfg), block, 0, s, a);
        return;
    }
    switch (tile_dt_of(a.d)) {
        case 1: launch_ratio_tile<1, KIND, NT>(a, grad, s); break;
        case 2: launch_ratio_tile<2, KIND, NT>(a, grad, s); break;
        case 4: launch_ratio_tile<4, KIND, NT>(a, grad, s); break;
        default: launch_ratio_tile<8, KIND, NT>(a, grad, s); break;
    }
}

// term counts with a compiled fast form: rbf (1), mix_rbf (6), mix_rq* (3)
static bool launch_ratio_kind(const RatioArgs &a, bool grad, hipStream_t s) {
    const int nt = a.kp.n_terms;
    switch (a.kind) {
        case SMMD_KIND_RBF:
            if (nt == 1) launch_ratio_sweep<SMMD_KIND_RBF, 1>(a, grad, s);
            else if (nt == 6) launch_ratio_sweep<SMMD_KIND_RBF, 6>(a, grad, s);
            else launch_ratio_sweep<SMMD_KIND_RBF, 0>(a, grad, s);
            return true;
        case SMMD_KIND_RQ:
            if (nt == 3) launch_ratio_sweep<SMMD_KIND_RQ, 3>(a, grad, s);
            else launch_ratio_sweep<SMMD_KIND_RQ, 0>(a, grad, s);
            return true;
        case SMMD_KIND_DISTANCE: launch_ratio_sweep<SMMD_KIND_DISTANCE, 0>(a, grad, s); return true;
        case SMMD_KIND_DOT: launch_ratio_sweep<SMMD_KIND_DOT, 0>(a, grad, s); return true;
    }
    return false;
}

// smmd_mmd.hip's make_kparams (file-local there)
static bool ratio_kparams(const smmd_kernel_desc *desc, KParams &kp) {
    memset(&kp, 0, sizeof(kp));
    if (desc->kind == SMMD_KIND_RBF || desc->kind == SMMD_KIND_RQ) {
        if (desc->n_terms < 1 || desc->n_terms > SMMD_MAX_TERMS) return false;
        kp.n_terms = desc->n_terms;
        for (int t = 0; t < desc->n_terms; ++t) {
            const double s = desc->param[t];
            if (!(s > 0)) return false;
            if (desc->kind == SMMD_KIND_RBF) {
                kp.c1[t] = (float)(-(1.0 / (2.0 * s * s)));   // -gamma, mmd.py:69-70
            } else {
                kp.c1[t] = (float)(2.0 * s);                   // 2.*alpha, mmd.py:166
                kp.c2[t] = (float)(-s);                        // -alpha, mmd.py:167
            }
            kp.wt[t] = (float)desc->wt[t];
        }
        kp.add_dot = (desc->kind == SMMD_KIND_RQ) ? (float)desc->add_dot : 0.f;
        return true;
    }
    return desc->kind == SMMD_KIND_DISTANCE || desc->kind == SMMD_KIND_DOT;
}

}  // namespace smmd

using namespace smmd;

extern "C" {

size_t smmd_mmd2_ratio_workspace_bytes(int m, int d) {
    if (m < 2 || d < 1) return 0;
    RatioArgs a;
    memset(&a, 0, sizeof(a));
    return ratio_plan(m, d, a, nullptr);
}

smmd_status smmd_mmd2_ratio_fwd(const smmd_kernel_desc *desc, const float *X, const float *Y,
                                int m, int d, int biased, double min_var_est, float *out,
                                float *grad_mmd2_x, float *grad_mmd2_y, float *grad_var_x,
                                float *grad_var_y, void *ws, size_t ws_bytes,
                                smmd_stream_t stream) {
    if (!desc || !X || !Y || !out || m < 2 || d < 1) return SMMD_EINVAL;
    const int ng = (grad_mmd2_x != nullptr) + (grad_mmd2_y != nullptr) + (grad_var_x != nullptr) +
                   (grad_var_y != nullptr);
    if (ng != 0 && ng != 4) return SMMD_EINVAL;
    if ((int64_t)2 * ((int64_t)m + RT) * ((int64_t)d + 4) > 0x7fffffff) return SMMD_EINVAL;
    RatioArgs a;
    memset(&a, 0, sizeof(a));
    if (!ratio_kparams(desc, a.kp)) return SMMD_EINVAL;
    const size_t need = ratio_plan(m, d, a, (char *)ws);
    if (!ws || ws_bytes < need) return SMMD_EWORKSPACE;
    if (a.n_cc > 0x7fffffff / (2 * a.nts)) return SMMD_EINVAL;     // the tile path's 1-D grid
    if (a.mfma && (2 * a.nts > 65535 || a.nfg > 65535)) return SMMD_EINVAL;
    a.X = X;
    a.Y = Y;
    a.kind = desc->kind;
    a.tanh_in = desc->tanh_inputs ? 1 : 0;
    a.has_const = desc->has_const_diag ? 1 : 0;
    a.const_diag = desc->const_diag;
    a.biased = biased ? 1 : 0;
    a.min_var = min_var_est;
    a.out = out;
    a.gm_x = grad_mmd2_x; a.gm_y = grad_mmd2_y;
    a.gv_x = grad_var_x; a.gv_y = grad_var_y;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ratio_prep_kernel, dim3((a.Rp + 3) / 4), dim3(256), 0, s, a);
    if (!launch_ratio_kind(a, false, s)) return SMMD_EINVAL;
    hipLaunchKernelGGL(ratio_rowsum_kernel, dim3((a.Rp + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ratio_final_kernel, dim3(1), dim3(256), 0, s, a);
    if (ng) {
        launch_ratio_kind(a, true, s);
        const size_t n = (size_t)a.Rp * a.dp;
        hipLaunchKernelGGL(ratio_gradsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                           a);
    }
    const size_t n16 = need / 16;
    const size_t cb = (n16 + 255) / 256;
    hipLaunchKernelGGL(ratio_clear_kernel, dim3((unsigned)(cb < 2048 ? (cb ? cb : 1) : 2048)),
                       dim3(256), 0, s, (uint4 *)ws, n16);
    return last_launch_status();
}

smmd_status smmd_mmd2_ratio_bwd(const float *out, const float *g_mmd2, const float *g_ratio,
                                const float *g_var, const float *grad_mmd2_x,
                                const float *grad_mmd2_y, const float *grad_var_x,
                                const float *grad_var_y, int m, int d, float *dX, float *dY,
                                smmd_stream_t stream) {
    if (!out || !grad_mmd2_x || !grad_mmd2_y || !grad_var_x || !grad_var_y || !dX || !dY ||
        m < 2 || d < 1)
        return SMMD_EINVAL;
    RatioBwdArgs b;
    b.out = out; b.g_mmd2 = g_mmd2; b.g_ratio = g_ratio; b.g_var = g_var;
    b.gm_x = grad_mmd2_x; b.gm_y = grad_mmd2_y; b.gv_x = grad_var_x; b.gv_y = grad_var_y;
    b.dX = dX; b.dY = dY;
    b.n = (size_t)m * d;
    if ((2 * b.n + 255) / 256 > 0x7fffffff) return SMMD_EINVAL;
    hipLaunchKernelGGL(ratio_bwd_kernel, dim3((unsigned)((2 * b.n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, b);
    return last_launch_status();
}

}  // extern "C"
