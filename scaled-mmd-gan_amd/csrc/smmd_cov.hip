// smmd_cov.hip -- mean and covariance of gathered code rows for the FID
// (gan/compute_scores.py:193-197: part.mean(axis=0), np.cov(part, rowvar=False)
// for part = codes[index]), gfx950.
//
// Four launches on the caller's stream, no floating-point atomics, every
// reduction in a fixed order (two runs give the same bits):
//   1. cov_colsum_kernel    double column sums of the gathered rows, one
//                           partial row per slab of CS_ROWS rows
//   2. cov_mean_kernel      the partials in slab order -> mean, the f32 shift
//                           c = float(mean) and delta = mean - c
//   3. cov_moment_kernel    S = sum_r (x_r - c)(x_r - c)^T on
//                           v_mfma_f32_32x32x2_f32: 64 x 64 block tiles on or
//                           above the diagonal, split over row slices; f32
//                           running sums for the 32 rows of a step, then folded
//                           into double registers; one double slab per slice
//   4. cov_finish_kernel    slabs in slice order, cov = (S - n delta delta^T)
//                           / (n - 1), the tile and its mirror from the same
//                           values
// The gather never materialises: kernels 1 and 3 read codes[index[r]] in place.
#include "smmd_common.hpp"

namespace {

using namespace smmd;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CT = 64;            // block tile: CT x CT outputs, 4 waves of 32 x 32
// rows staged per step, and the length of an f32 run: every step's sums are
// folded into the double accumulators.  The error of a run of all-positive
// products (the diagonal) grows with its length: against float64, 256-row runs
// gave 1.2e-6 of max |cov|, 64-row runs 5.1e-7, 32-row runs 2.5e-7, for 16
// conversions and double adds per 16 MFMAs (+3 % time at 25 000 x 2048).
constexpr int KC = 32;
constexpr int MIN_STEPS = 16;     // a slice is at least 512 rows (or all of them)
constexpr int TARGET_BLOCKS = 1024;
constexpr int CS_ROWS = 128;      // rows per column-sum slab
constexpr int CS_MAX_SLABS = 32768;

struct CovPlan {
    int nt;              // column tiles: ceil(dim / CT)
    long long ntri;      // tiles on or above the diagonal
    int slices;          // row slices of the second moment
    int steps;           // KC-row steps per slice
    int cs_rows;         // rows per column-sum slab
    int cs_slabs;
    size_t off_c, off_delta, off_part, off_slab, bytes;
};

inline CovPlan cov_plan(int n, int dim) {
    CovPlan p{};
    p.nt = (dim + CT - 1) / CT;
    p.ntri = (long long)p.nt * (p.nt + 1) / 2;
    const int nsteps = (n + KC - 1) / KC;
    long long want = (TARGET_BLOCKS + p.ntri - 1) / p.ntri;
    const int cap = (nsteps + MIN_STEPS - 1) / MIN_STEPS;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    p.steps = (int)((nsteps + want - 1) / want);
    p.slices = (nsteps + p.steps - 1) / p.steps;
    p.cs_rows = CS_ROWS;
    if ((n + p.cs_rows - 1) / p.cs_rows > CS_MAX_SLABS)
        p.cs_rows = (n + CS_MAX_SLABS - 1) / CS_MAX_SLABS;
    p.cs_slabs = (n + p.cs_rows - 1) / p.cs_rows;
    size_t o = 0;
    p.off_c = o;
    o += align_up((size_t)dim * sizeof(float), 256);
    p.off_delta = o;
    o += align_up((size_t)dim * sizeof(double), 256);
    p.off_part = o;
    o += align_up((size_t)p.cs_slabs * dim * sizeof(double), 256);
    p.off_slab = o;
    o += (size_t)p.slices * (size_t)p.ntri * CT * CT * sizeof(double);
    p.bytes = o;
    return p;
}

__device__ __forceinline__ long long row_of(const int64_t *__restrict__ index, int r) {
    return index ? (long long)index[r] : (long long)r;
}

// ---- 1. column sums ---------------------------------------------------------
// grid (ceil(dim / 256), slabs); thread = column; rows of the slab ascending
__global__ __launch_bounds__(256) void cov_colsum_kernel(const float *__restrict__ codes, int dim,
                                                         const int64_t *__restrict__ index, int n,
                                                         int rows_per, double *__restrict__ part) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * rows_per;
    const int r1 = min(n, r0 + rows_per);
    const int cc = col < dim ? col : 0;
    double s = 0.0;
    for (int r = r0; r < r1; r += 8) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int rr = r + j < r1 ? r + j : r0;
            t[j] = codes[(size_t)row_of(index, rr) * dim + cc];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (r + j < r1) s += (double)t[j];
    }
    if (col < dim) part[(size_t)blockIdx.y * dim + col] = s;
}

// ---- 2. mean, shift, residual ------------------------------------------------
__global__ __launch_bounds__(256) void cov_mean_kernel(const double *__restrict__ part, int dim,
                                                       int slabs, int n, double *__restrict__ mean,
                                                       float *__restrict__ c,
                                                       double *__restrict__ delta) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= dim) return;
    double s = 0.0;
    for (int b = 0; b < slabs; b += 8) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = b + j < slabs ? part[(size_t)(b + j) * dim + col] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (b + j < slabs) s += t[j];
    }
    const double m = s / (double)n;
    const float cf = (float)m;
    mean[col] = m;
    c[col] = cf;
    delta[col] = m - (double)cf;
}

// block tile t of the upper triangle (row-major over bi <= bj) -> (bi, bj)
__device__ __forceinline__ void tri_tile(long long t, int nt, int &bi, int &bj) {
    int i = 0, len = nt;
    while (t >= len) {
        t -= len;
        ++i;
        --len;
    }
    bi = i;
    bj = i + (int)t;
}

// ---- 3. centred second moment -------------------------------------------------
// One block = one 64 x 64 tile of one row slice; 4 waves, wave (wi, wj) owns
// the 32 x 32 quadrant.  Each step stages KC centred rows of the tile's two
// column panels in LDS ([k][64], the rows as they lie in memory), 16 MFMAs per
// wave read them (A[i][k] = panel_i[k][i], B[k][j] = panel_j[k][j]: lane l
// takes row k + (l >> 5), column l & 31).  The next step's rows are in flight
// in registers meanwhile, their row offsets fetched one step earlier still.
// VEC: dim % 4 == 0 and codes 16-byte aligned -> float4 loads; otherwise
// scalar loads (rows are then not 16-byte aligned).
template <bool VEC>
struct Stager {
    static constexpr int NR = VEC ? 2 : 8;      // rows per thread and step
    static constexpr int RS = VEC ? 16 : 4;     // row stride between them
    static constexpr int W = VEC ? 4 : 1;       // floats per load
};

template <bool VEC>
__global__ __launch_bounds__(256) void cov_moment_kernel(
    const float *__restrict__ codes, int dim, const int64_t *__restrict__ index, int n,
    const float *__restrict__ c, int nt, long long ntri, int steps, double *__restrict__ slab) {
    using S = Stager<VEC>;
    constexpr int NR = S::NR, RS = S::RS, W = S::W;
    __shared__ float sm[2][KC][CT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const long long work = xcd_order(blockIdx.x, gridDim.x);
    const int slice = (int)(work / ntri);
    const long long tile = work - (long long)slice * ntri;
    int bi, bj;
    tri_tile(tile, nt, bi, bj);

    const int rbeg = slice * steps * KC;
    const int rend = min(n, rbeg + steps * KC);
    const int nsteps = (rend - rbeg + KC - 1) / KC;

    // this thread's columns of the two panels and their shifts
    const int lc = VEC ? (tid & 15) * 4 : (tid & 63);   // column inside the panel
    const int lr = VEC ? (tid >> 4) : (tid >> 6);       // first row inside the step
    const int ca = bi * CT + lc, cb = bj * CT + lc;
    const bool oka = ca < dim, okb = cb < dim;          // VEC: dim % 4 == 0, all 4 or none
    const int cca = oka ? ca : 0, ccb = okb ? cb : 0;
    float sha[W], shb[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
        sha[e] = oka ? c[cca + e] : 0.f;
        shb[e] = okb ? c[ccb + e] : 0.f;
    }

    auto load_off = [&](int r0, size_t (&off)[NR]) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int r = r0 + lr + RS * j;
            off[j] = r < rend ? (size_t)row_of(index, r) * dim : 0;   // past the end: row 0, zeroed below
        }
    };
    auto load_data = [&](const size_t (&off)[NR], float (&ra)[NR][W], float (&rb)[NR][W]) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if constexpr (VEC) {
                const float4 va = *reinterpret_cast<const float4 *>(codes + off[j] + cca);
                const float4 vb = *reinterpret_cast<const float4 *>(codes + off[j] + ccb);
                ra[j][0] = va.x, ra[j][1] = va.y, ra[j][2] = va.z, ra[j][3] = va.w;
                rb[j][0] = vb.x, rb[j][1] = vb.y, rb[j][2] = vb.z, rb[j][3] = vb.w;
            } else {
                ra[j][0] = codes[off[j] + cca];
                rb[j][0] = codes[off[j] + ccb];
            }
        }
    };

    size_t off[NR];
    float ra[NR][W], rb[NR][W];
    load_off(rbeg, off);
    load_data(off, ra, rb);
    load_off(rbeg + KC, off);

    f32x16 acc = {0};
    double dacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dacc[i] = 0.0;

    const int kh = lane >> 5, l31 = lane & 31;
    for (int st = 0; st < nsteps; ++st) {
        const int r0 = rbeg + st * KC;
        __syncthreads();                       // the last step's reads are done
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int k = lr + RS * j;
            const bool rok = r0 + k < rend;
            float wa[W], wb[W];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                wa[e] = (rok && oka) ? ra[j][e] - sha[e] : 0.f;
                wb[e] = (rok && okb) ? rb[j][e] - shb[e] : 0.f;
            }
            if constexpr (VEC) {
                *reinterpret_cast<float4 *>(&sm[0][k][lc]) = make_float4(wa[0], wa[1], wa[2], wa[3]);
                *reinterpret_cast<float4 *>(&sm[1][k][lc]) = make_float4(wb[0], wb[1], wb[2], wb[3]);
            } else {
                sm[0][k][lc] = wa[0];
                sm[1][k][lc] = wb[0];
            }
        }
        __syncthreads();
        // rows of step st + 1 (offsets already here), offsets of step st + 2
        load_data(off, ra, rb);
        load_off(r0 + 2 * KC, off);
#pragma unroll
        for (int k = 0; k < KC; k += 2) {
            const float a = sm[0][k + kh][wi * 32 + l31];
            const float b = sm[1][k + kh][wj * 32 + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            dacc[i] += (double)acc[i];
            acc[i] = 0.f;
        }
    }

    // C/D map of the 32x32 f32 MFMA: column = lane & 31, row = (reg & 3) +
    // 8 (reg >> 2) + 4 (lane >> 5)
    double *out = slab + ((size_t)slice * (size_t)ntri + (size_t)tile) * (CT * CT);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = wi * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
        out[row * CT + wj * 32 + l31] = dacc[i];
    }
}

// ---- 4. slabs -> covariance ---------------------------------------------------
// One block per tile.  The summed tile goes through LDS so that the tile and
// its mirror are both written along rows of cov.
__global__ __launch_bounds__(256) void cov_finish_kernel(const double *__restrict__ slab,
                                                         const double *__restrict__ delta, int dim,
                                                         int n, int nt, long long ntri, int slices,
                                                         double *__restrict__ cov) {
    __shared__ double T[CT][CT + 1];
    const long long tile = blockIdx.x;
    int bi, bj;
    tri_tile(tile, nt, bi, bj);
    const double inv = 1.0 / (double)(n - 1);
    for (int e = threadIdx.x; e < CT * CT; e += 256) {
        const int i = e >> 6, j = e & 63;
        double s = 0.0;
        for (int sl = 0; sl < slices; ++sl)
            s += slab[((size_t)sl * (size_t)ntri + (size_t)tile) * (CT * CT) + e];
        const int gi = bi * CT + i, gj = bj * CT + j;
        double v = 0.0;
        if (gi < dim && gj < dim) v = (s - (double)n * (delta[gi] * delta[gj])) * inv;
        T[i][j] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CT * CT; e += 256) {
        const int a = e >> 6, b = e & 63;
        if (bi == bj) {
            // diagonal tile: both halves from the elements on or above the diagonal
            const int gi = bi * CT + a, gj = bi * CT + b;
            if (gi < dim && gj < dim) cov[(size_t)gi * dim + gj] = a <= b ? T[a][b] : T[b][a];
        } else {
            const int gi = bi * CT + a, gj = bj * CT + b;
            if (gi < dim && gj < dim) cov[(size_t)gi * dim + gj] = T[a][b];
            const int mi = bj * CT + a, mj = bi * CT + b;      // mirror: cov[J + a][I + b]
            if (mi < dim && mj < dim) cov[(size_t)mi * dim + mj] = T[b][a];
        }
    }
}

}  // namespace

extern "C" {

size_t smmd_code_moments_workspace_bytes(int n, int dim) {
    if (n < 2 || dim < 1) return 0;
    return cov_plan(n, dim).bytes;
}

smmd_status smmd_code_moments(const float *codes, int n_rows, int dim, const int64_t *index, int n,
                              double *mean, double *cov, void *ws, size_t ws_bytes,
                              smmd_stream_t stream) {
    if (!codes || !mean || !cov || n_rows < 1 || dim < 1 || n < 2) return SMMD_EINVAL;
    if (!index && n > n_rows) return SMMD_EINVAL;
    const CovPlan p = cov_plan(n, dim);
    if ((long long)p.slices * p.ntri > 0x7fffffffLL) return SMMD_EINVAL;
    if (!ws || ws_bytes < p.bytes) return SMMD_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws;
    float *c = (float *)(w + p.off_c);
    double *delta = (double *)(w + p.off_delta);
    double *part = (double *)(w + p.off_part);
    double *slab = (double *)(w + p.off_slab);
    const unsigned cblocks = (unsigned)((dim + 255) / 256);

    hipLaunchKernelGGL(cov_colsum_kernel, dim3(cblocks, (unsigned)p.cs_slabs), dim3(256), 0, s,
                       codes, dim, index, n, p.cs_rows, part);
    hipLaunchKernelGGL(cov_mean_kernel, dim3(cblocks), dim3(256), 0, s, part, dim, p.cs_slabs, n,
                       mean, c, delta);
    const unsigned blocks = (unsigned)(p.slices * p.ntri);
    if ((dim & 3) == 0 && ((uintptr_t)codes & 15) == 0)
        hipLaunchKernelGGL(cov_moment_kernel<true>, dim3(blocks), dim3(256), 0, s, codes, dim,
                           index, n, c, p.nt, p.ntri, p.steps, slab);
    else
        hipLaunchKernelGGL(cov_moment_kernel<false>, dim3(blocks), dim3(256), 0, s, codes, dim,
                           index, n, c, p.nt, p.ntri, p.steps, slab);
    hipLaunchKernelGGL(cov_finish_kernel, dim3((unsigned)p.ntri), dim3(256), 0, s, slab, delta, dim,
                       n, p.nt, p.ntri, p.slices, cov);
    return last_launch_status();
}

}  // extern "C"
