// smmd_fid_sqrt.hip -- the FID's spectral step on the f64 matrix cores:
// tr sqrt(cov_g cov_r) of two symmetric PSD d x d double matrices by the
// coupled Newton-Schulz iteration (no eigenvectors, no host round trip), gfx950.
//
// For a PSD A: c = |A|_F, Y0 = A / c + delta I, Z0 = I, then `iters` times
//     T = 1.5 I - 0.5 Z Y;   Y <- Y T;   Z <- T Z          (Y -> sqrt(Y0))
// with full products and no symmetrisation inside the loop (symmetrising Y, Z
// and T every iteration overflowed in a float64 mirror; plain products converge
// and stay put).  The shift delta keeps the rounding-level negative eigenvalues
// of a singular A inside the basin.  Three stages:
//   1. Y1 = Y(cov_g)                       S = sqrt(c1) Y1
//   2. M  = c1 (Y1 cov_r) Y1               = S cov_r S, and |M|_F from the
//                                            second product's epilogue
//   3. Y3 = Y(M),  tr_sqrt = sqrt(c3) tr Y3
// and per stage the residual |Y^2 - Y0|_F (one more product, nothing stored).
//
// Launches, all plain grids on the caller's stream (no float atomics, no
// tickets, no host read: c1 and c3 stay in the workspace):
//   fs_sqsum_kernel    sum of squares of each 128 x 128 tile -> one partial each
//   fs_init_kernel     the partials in index order -> c; Y = A / c + delta I,
//                      Z = I
//   fs_gemm_kernel     C = A B on v_mfma_f64_16x16x4_f64 with the epilogues
//                      EPI_T (1.5 I - 0.5 AB), EPI_PLAIN, EPI_SCALE_SQ (c1 AB
//                      and its tile's sum of squares), EPI_RESID ((AB - Y0)^2
//                      summed, not stored); blockIdx.z picks one of two
//                      products, so Y T and T Z are one launch
//   fs_finish_kernel   trace, the residual partials in index order -> out4
//
// The GEMM: one block = one 128 x 128 tile of C, 4 waves of 64 x 64 (4 x 4
// MFMA tiles, 64 accumulator doubles per lane).  K goes in chunks of 8 through
// double-buffered LDS: the A panel as [row][k] with a pitch of 10 doubles, the
// B panel as [k][column] with a pitch of 144, so that a fragment read (lane l:
// row or column l & 15, k = l >> 4) touches every bank pair once per 32 lanes.
// The next chunk is in flight in registers during the 32 MFMAs of the current
// one; one barrier per chunk.  Rows, columns and k past d are loaded from a
// clamped address and zeroed at the LDS store: no branch in the MFMA loop.
// VEC: d even and 16-byte aligned operands -> double2 loads, else scalar.
#include "smmd_common.hpp"

namespace {

using namespace smmd;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 128;          // block tile
constexpr int KC = 8;            // k per LDS chunk: two MFMA k-steps
constexpr int SA = KC + 2;       // pitch of an A row in LDS, doubles
constexpr int SB = BT + 16;      // pitch of a B row in LDS, doubles
constexpr int N_BUF = 6;         // d x d buffers: Y, Z, T, Y', Z', M

enum { EPI_PLAIN, EPI_T, EPI_SCALE_SQ, EPI_RESID };

struct FsPlan {
    int nt;                      // tiles per side
    int np;                      // partials per reduction: nt * nt
    size_t off_part[3], off_buf, buf_bytes, bytes;
};

inline FsPlan fs_plan(int dim) {
    FsPlan p{};
    p.nt = (dim + BT - 1) / BT;
    p.np = p.nt * p.nt;
    size_t o = 256;              // the scalars: c1, c3
    for (int i = 0; i < 3; ++i) {
        p.off_part[i] = o;
        o += align_up((size_t)p.np * sizeof(double), 256);
    }
    p.off_buf = o;
    p.buf_bytes = align_up((size_t)dim * dim * sizeof(double), 256);
    p.bytes = o + N_BUF * p.buf_bytes;
    return p;
}

struct GemmArgs {
    const double *A0, *B0, *A1, *B1;   // the operands of product 0 and 1 (blockIdx.z)
    double *C0, *C1;
    const double *R;       // EPI_RESID: the stage's input matrix
    const double *c;       // EPI_SCALE_SQ: the factor c1; EPI_RESID: the norm of R
    double *part;          // EPI_SCALE_SQ / EPI_RESID: one partial per tile
    double delta;
    int d, nt;
};

__device__ __forceinline__ double inv_norm(double c) { return c > 0.0 ? 1.0 / c : 0.0; }

// the scaled and shifted input, the same expression wherever it is formed
__device__ __forceinline__ double shifted(double a, double inv, double delta, bool diag) {
    double v = a * inv;
    if (diag) v += delta;
    return v;
}

// sqrt of the partials' sum in index order; every thread of the block gets it
__device__ __forceinline__ double norm_of(const double *__restrict__ part, int np, double *red) {
    return sqrt(block_sum<4>(strided_sum(part, (int)threadIdx.x, np, 256), red));
}

template <bool VEC, int EPI>
__global__ __launch_bounds__(256) void fs_gemm_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) double sA[2][BT][SA];
    __shared__ __attribute__((aligned(16))) double sB[2][KC][SB];
    __shared__ double red[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const bool second = blockIdx.z != 0;
    const double *__restrict__ A = second ? g.A1 : g.A0;
    const double *__restrict__ B = second ? g.B1 : g.B0;
    double *__restrict__ C = second ? g.C1 : g.C0;
    const int d = g.d;
    // XCD-aware: one XCD takes whole rows of tiles, which share an A panel
    const int work = xcd_order(blockIdx.x, gridDim.x);
    const int bi = work / g.nt, bj = work - bi * g.nt;

    // loaders: A rows ar and ar + 64, k pair akp; B k rows bk and bk + 4,
    // column pair bcp
    const int akp = (tid & 3) * 2, ar = tid >> 2;
    const int bcp = (tid & 63) * 2, bk = tid >> 6;
    const int bcol = bj * BT + bcp;
    size_t aoff[2];
    bool aok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = bi * BT + ar + 64 * j;
        aok[j] = row < d;
        aoff[j] = aok[j] ? (size_t)row * d : 0;
    }

    double ra[2][2], rb[2][2];
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + akp;
            const bool ok0 = aok[j] && k < d, ok1 = aok[j] && k + 1 < d;
            if constexpr (VEC) {
                const double2 v = *reinterpret_cast<const double2 *>(A + (ok0 ? aoff[j] + k : 0));
                ra[j][0] = v.x, ra[j][1] = v.y;
            } else {
                ra[j][0] = A[ok0 ? aoff[j] + k : 0];
                ra[j][1] = A[ok1 ? aoff[j] + k + 1 : 0];
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + bk + 4 * j;
            const size_t off = (size_t)k * d + bcol;
            const bool ok0 = k < d && bcol < d, ok1 = k < d && bcol + 1 < d;
            if constexpr (VEC) {
                const double2 v = *reinterpret_cast<const double2 *>(B + (ok0 ? off : 0));
                rb[j][0] = v.x, rb[j][1] = v.y;
            } else {
                rb[j][0] = B[ok0 ? off : 0];
                rb[j][1] = B[ok1 ? off + 1 : 0];
            }
        }
    };
    // what lies past d becomes 0 here (VEC: d is even, a pair is in or out)
    auto store = [&](int k0, int buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + akp;
            const bool ok0 = aok[j] && k < d, ok1 = aok[j] && k + 1 < d;
            *reinterpret_cast<double2 *>(&sA[buf][ar + 64 * j][akp]) =
                make_double2(ok0 ? ra[j][0] : 0.0, ok1 ? ra[j][1] : 0.0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + bk + 4 * j;
            const bool ok0 = k < d && bcol < d, ok1 = k < d && bcol + 1 < d;
            *reinterpret_cast<double2 *>(&sB[buf][bk + 4 * j][bcp]) =
                make_double2(ok0 ? rb[j][0] : 0.0, ok1 ? rb[j][1] : 0.0);
        }
    };

    f64x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};

    // fragments of v_mfma_f64_16x16x4_f64: A[i = l & 15][k = l >> 4],
    // B[k = l >> 4][j = l & 15]
    const int fl = lane & 15, fk = lane >> 4;
    const int nch = (d + KC - 1) / KC;
    load(0);
    store(0, 0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        load((ch + 1) * KC);                  // past the last chunk: address 0, unused
#pragma unroll
        for (int ks = 0; ks < KC; ks += 4) {
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = sA[buf][wi * 64 + m * 16 + fl][ks + fk];
#pragma unroll
            for (int n = 0; n < 4; ++n) b[n] = sB[buf][ks + fk][wj * 64 + n * 16 + fl];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        // the other buffer: its readers passed the last barrier (after the
        // last chunk it takes zeros that nobody reads: no branch here)
        store((ch + 1) * KC, buf ^ 1);
        __syncthreads();
    }

    // C/D map of the f64 16x16x4 MFMA: column = l & 15, row = 4 reg + (l >> 4)
    double scale = 1.0, inv = 0.0, sq = 0.0;
    if constexpr (EPI == EPI_SCALE_SQ) scale = *g.c;
    if constexpr (EPI == EPI_RESID) inv = inv_norm(*g.c);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bi * BT + wi * 64 + m * 16 + 4 * r + fk;
                const int col = bj * BT + wj * 64 + n * 16 + fl;
                if (row >= d || col >= d) continue;
                const size_t o = (size_t)row * d + col;
                double v = acc[m][n][r];
                if constexpr (EPI == EPI_PLAIN) {
                    C[o] = v;
                } else if constexpr (EPI == EPI_T) {
                    C[o] = (row == col ? 1.5 : 0.0) - 0.5 * v;
                } else if constexpr (EPI == EPI_SCALE_SQ) {
                    v *= scale;
                    C[o] = v;
                    sq += v * v;
                } else {
                    v -= shifted(g.R[o], inv, g.delta, row == col);
                    sq += v * v;
                }
            }
    if constexpr (EPI == EPI_SCALE_SQ || EPI == EPI_RESID) {
        sq = block_sum<4>(sq, red);
        if (tid == 0) g.part[work] = sq;
    }
}

// ---- sum of squares per 128 x 128 tile (the partials of |A|_F) ----------------
__global__ __launch_bounds__(256) void fs_sqsum_kernel(const double *__restrict__ A, int d, int nt,
                                                       double *__restrict__ part) {
    __shared__ double red[4];
    const int bi = blockIdx.x / nt, bj = blockIdx.x - bi * nt;
    const int col = bj * BT + (threadIdx.x & 127);
    const int r0 = bi * BT + (threadIdx.x >> 7);
    double s = 0.0;
    if (col < d)
        for (int r = r0; r < min(d, (bi + 1) * BT); r += 2) {
            const double v = A[(size_t)r * d + col];
            s += v * v;
        }
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- Y = A / c + delta I, Z = I, c = |A|_F from the partials ------------------
__global__ __launch_bounds__(256) void fs_init_kernel(const double *__restrict__ A, int d,
                                                      const double *__restrict__ part, int np,
                                                      double delta, double *__restrict__ Y,
                                                      double *__restrict__ Z,
                                                      double *__restrict__ c_out) {
    __shared__ double red[4];
    const double c = norm_of(part, np, red);          // the same bits in every block
    const double inv = inv_norm(c);
    const size_t total = (size_t)d * d, step = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        const size_t i = e / d;
        const bool diag = e - i * d == i;
        Y[e] = shifted(A[e], inv, delta, diag);
        Z[e] = diag ? 1.0 : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *c_out = c;
}

// ---- out4 = {sqrt(c3) tr Y, residual 1, residual 3, c3} -------------------------
__global__ __launch_bounds__(256) void fs_finish_kernel(const double *__restrict__ Y, int d,
                                                        const double *__restrict__ scal,
                                                        const double *__restrict__ part1,
                                                        const double *__restrict__ part3, int np,
                                                        double *__restrict__ out4) {
    __shared__ double red[4];
    double t = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) t += Y[(size_t)i * d + i];
    t = block_sum<4>(t, red);
    const double r1 = norm_of(part1, np, red);
    const double r3 = norm_of(part3, np, red);
    if (threadIdx.x == 0) {
        const double c3 = scal[1];
        out4[0] = sqrt(c3) * t;
        out4[1] = r1;
        out4[2] = r3;
        out4[3] = c3;
    }
}

template <int EPI>
smmd_status fs_gemm(bool vec, const GemmArgs &g, int products, hipStream_t s) {
    const dim3 grid((unsigned)(g.nt * g.nt), 1, (unsigned)products);
    if (vec)
        hipLaunchKernelGGL((fs_gemm_kernel<true, EPI>), grid, dim3(256), 0, s, g);
    else
        hipLaunchKernelGGL((fs_gemm_kernel<false, EPI>), grid, dim3(256), 0, s, g);
    return last_launch_status();
}

inline bool fs_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t smmd_fid_trace_sqrt_workspace_bytes(int dim) {
    if (dim < 1) return 0;
    return fs_plan(dim).bytes;
}

smmd_status smmd_fid_trace_sqrt(const double *cov_g, const double *cov_r, int dim, double delta,
                                int iters, double *out4, void *ws, size_t ws_bytes,
                                smmd_stream_t stream) {
    if (!cov_g || !cov_r || !out4 || dim < 1 || !(delta > 0.0) || iters < 1) return SMMD_EINVAL;
    const FsPlan p = fs_plan(dim);
    if (!ws || ws_bytes < p.bytes) return SMMD_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws;
    double *scal = (double *)w;                       // c1, c3
    double *part_n = (double *)(w + p.off_part[0]);   // |A|_F of the running stage
    double *part_r[2] = {(double *)(w + p.off_part[1]), (double *)(w + p.off_part[2])};
    double *buf[N_BUF];
    for (int i = 0; i < N_BUF; ++i) buf[i] = (double *)(w + p.off_buf + i * p.buf_bytes);
    const bool vec = (dim & 1) == 0 && fs_aligned16(cov_g) && fs_aligned16(cov_r) && fs_aligned16(ws);
    // the element-wise pass: 8 elements per thread, at most 2048 blocks
    const size_t want = ((size_t)dim * dim + 2047) / 2048;
    const unsigned init_blocks = (unsigned)(want < 2048 ? want : 2048);

    GemmArgs g{};
    g.d = dim;
    g.nt = p.nt;
    g.delta = delta;
    double *Y = buf[0], *Z = buf[1], *T = buf[2], *Y2 = buf[3], *Z2 = buf[4], *M = buf[5];
    smmd_status e;

    // Y(src): src's partials are in part_n; leaves the root in Y, its residual's
    // partials in part_r[which]
    auto stage = [&](const double *src, int which) -> smmd_status {
        hipLaunchKernelGGL(fs_init_kernel, dim3(init_blocks), dim3(256), 0, s, src, dim, part_n,
                           p.np, delta, Y, Z, scal + which);
        if ((e = last_launch_status()) != SMMD_OK) return e;
        for (int it = 0; it < iters; ++it) {
            g.A0 = Z, g.B0 = Y, g.C0 = T;
            if ((e = fs_gemm<EPI_T>(vec, g, 1, s)) != SMMD_OK) return e;
            g.A0 = Y, g.B0 = T, g.C0 = Y2;
            g.A1 = T, g.B1 = Z, g.C1 = Z2;
            // the last Z has no reader
            if ((e = fs_gemm<EPI_PLAIN>(vec, g, it + 1 < iters ? 2 : 1, s)) != SMMD_OK) return e;
            double *t = Y; Y = Y2; Y2 = t;
            t = Z; Z = Z2; Z2 = t;
        }
        g.A0 = Y, g.B0 = Y, g.C0 = nullptr;
        g.R = src, g.c = scal + which, g.part = part_r[which];
        return fs_gemm<EPI_RESID>(vec, g, 1, s);
    };

    hipLaunchKernelGGL(fs_sqsum_kernel, dim3((unsigned)p.np), dim3(256), 0, s, cov_g, dim, p.nt,
                       part_n);
    if ((e = last_launch_status()) != SMMD_OK) return e;
    if ((e = stage(cov_g, 0)) != SMMD_OK) return e;
    // M = c1 (Y cov_r) Y and the partials of |M|_F
    g.A0 = Y, g.B0 = cov_r, g.C0 = T;
    if ((e = fs_gemm<EPI_PLAIN>(vec, g, 1, s)) != SMMD_OK) return e;
    g.A0 = T, g.B0 = Y, g.C0 = M;
    g.c = scal, g.part = part_n;
    if ((e = fs_gemm<EPI_SCALE_SQ>(vec, g, 1, s)) != SMMD_OK) return e;
    if ((e = stage(M, 1)) != SMMD_OK) return e;
    hipLaunchKernelGGL(fs_finish_kernel, dim3(1), dim3(256), 0, s, Y, dim, scal, part_r[0],
                       part_r[1], p.np, out4);
    return last_launch_status();
}

}  // extern "C"
