// smmd_cramer.hip -- the loss side of the Cramer GAN, gfx950 (MI355X): the
// row-wise energy-distance head with the row gradients of both losses, the
// penalty's seed and the seed's backward.  Latency-bound: a batch-64 head at
// dof_dim 256 reads 192 KiB.
//
// Reference: gan/core/cramer.py:81-92 (the critic lambda, the cramer and
// reddit_cramer losses), :88 / :92 / :96 (to_penalize and its gradient with
// respect to x_hat, the seed), gan/core/ops.py:203-206 (safer_norm).
//
// Work split.  A wave owns a row; a 256-thread block owns CR_ROWS = 16
// consecutive rows (wave w rows w, w + 4, ...), so batch 64 is 4 blocks.
//   * d <= 1024: the row's operands are read ONCE into registers, 4 consecutive
//     columns per lane and round of 256 columns.  Float4 form (d % 4 == 0 and
//     every base 16-byte aligned): lane l holds columns 256 r + 4 l .. + 3 of
//     round r.  Scalar form: columns 256 r + 64 j + l, j < 4.  One round
//     (d <= 256) and four rounds (d <= 1024) are separate instantiations, so a
//     narrow head does not carry the wide one's registers.
//   * all of a row's squared norms (six for the head, two norms and two dot
//     products for the seed's backward) go through ONE cross-lane butterfly:
//     four DPP steps inside a row of 16 lanes (quad permutes, half mirror,
//     mirror), then two swaps across the rows.  After every step the lanes of a
//     group hold the same bits, so a mirror adds what an xor would.
//   * the gradients are formed from the same registers and written with the
//     loads' own column map: nothing is read twice.
//   * d > 1024: the same wave streams the row in rounds of 256 columns, once
//     for the sums and a second time (a re-read, L2-resident) for the outputs.
//
// Arithmetic.  Inputs and outputs are fp32.  Differences, squared sums, the
// inverse norms and each output element are formed in double and rounded once
// on the store: with d = 1 every output is the difference of two saturated
// unit vectors, (1 - eps / 2 a^2) - (1 - eps / 2 h^2), which fp32 resolves to
// 1e-2 of its value; double costs nothing here (vector fp64 runs at the fp32
// rate on this part and the kernels wait on memory).  The seed's backward
// forms P_v w as (w n^2 - v (v.w)) / n^3 for the same reason, and the seed's
// forward saves its norms in double.
//
// Batch means are fixed-order: a double partial per block and loss published
// write-through, one arrival ticket per block, and the last block sums the
// partials in index order and leaves the ticket at rest (smmd_common.hpp, as
// gp_slope_fwd).  No float atomics: two runs give the same bits.
#include "smmd_common.hpp"

namespace smmd {

constexpr int CR_ROWS = 16;              // rows per block (4 per wave)
constexpr int CR_REG_MAX = 1024;         // widest register-resident row
constexpr size_t CR_WS_HEADER = 256;     // the arrival ticket (word 0)

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const long long v = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// N sums at once; every lane ends with the same bits of each
template <int N>
__device__ __forceinline__ void wave_sum_all(double (&s)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += dpp_f64<0xB1>(s[i]);     // quad_perm [1,0,3,2]
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += dpp_f64<0x4E>(s[i]);     // quad_perm [2,3,0,1]
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += dpp_f64<0x141>(s[i]);    // row_half_mirror
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += dpp_f64<0x140>(s[i]);    // row_mirror
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += __shfl_xor(s[i], 16, SMMD_WAVE);
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] += __shfl_xor(s[i], 32, SMMD_WAVE);
}

// A lane's four columns of the round starting at column `base`; zero past d.
template <bool VEC>
__device__ __forceinline__ void load4(const float *__restrict__ row, int d, int base, int lane,
                                      float (&v)[4]) {
    if (VEC) {
        const int c = base + 4 * lane;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < d) t = *reinterpret_cast<const float4 *>(row + c);     // d % 4 == 0
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = base + 64 * j + lane;
            v[j] = (c < d) ? row[c] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ row, int d, int base, int lane,
                                       const double (&o)[4]) {
    if (VEC) {
        const int c = base + 4 * lane;
        if (c < d)
            *reinterpret_cast<float4 *>(row + c) =
                make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = base + 64 * j + lane;
            if (c < d) row[c] = (float)o[j];
        }
    }
}

// A row's operands: NR rounds in registers (NR = 1, 4) or, NR = 0, one round
// at a time from memory.
template <int NR, bool VEC, int NOP>
struct RowOps {
    static constexpr int NG = NR ? NR : 1;
    const float *p[NOP];
    float v[NOP][NG][4];
    int d, lane;

    __device__ __forceinline__ int rounds() const { return NR ? NR : (d + 255) >> 8; }
    __device__ __forceinline__ void fetch(int r) {          // round r into slot (NR ? r : 0)
#pragma unroll
        for (int k = 0; k < NOP; ++k) load4<VEC>(p[k], d, r << 8, lane, v[k][NR ? r : 0]);
    }
};

// ---------------------------------------------------------------------------
// head
// ---------------------------------------------------------------------------
struct HeadArgs {
    const float *G, *G2, *X;
    float *out;              // [2] d_base, g_loss
    float *dD[3], *dGl[3];   // row gradients w.r.t. G, G2, X (NULL: not wanted)
    double *part;            // [2][blocks]
    unsigned *counter;
    int b, d, variant;
    double eps;
};

// inverse norms over b: i[0] g-g2, [1] g-x, [2] g2-x, [3] x, [4] g2, [5] g
__device__ __forceinline__ void head_emit(const HeadArgs &a, const double (&i)[6], float gf,
                                          float g2f, float xf, double (&o)[6]) {
    const double g = gf, g2 = g2f, x = xf;
    const double ugg2 = (g - g2) * i[0], ugx = (g - x) * i[1], ug2x = (g2 - x) * i[2];
    if (a.variant == 0) {                  // cramer.py:85-88
        o[0] = ugg2 - ugx;                 // d d_base / d g
        o[1] = -ugg2 - g2 * i[4];
        o[2] = ugx + x * i[3];
        o[3] = ugx - ugg2;                 // d g_loss / d g
        o[4] = ugg2 + ug2x;
        o[5] = -ugx - ug2x;
    } else {                               // cramer.py:90-92
        o[3] = ugx - ugg2 + g * i[5];
        o[4] = ugg2;
        o[5] = -ugx - x * i[3];
        o[0] = -o[3];
        o[1] = -o[4];
        o[2] = -o[5];
    }
}

template <int NR, bool VEC>
__global__ __launch_bounds__(256) void cramer_head_kernel(HeadArgs a) {
    constexpr int UNR = NR ? NR : 1;         // rounds unrolled: all of a register-resident row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = a.d;
    double acc_d = 0.0, acc_g = 0.0;
    for (int j = 0; j < CR_ROWS / 4; ++j) {
        const int row = blockIdx.x * CR_ROWS + 4 * j + wave;       // wave-uniform
        if (row >= a.b) break;
        const int64_t off = (int64_t)row * d;
        RowOps<NR, VEC, 3> R;
        R.p[0] = a.G + off;
        R.p[1] = a.G2 + off;
        R.p[2] = a.X + off;
        R.d = d;
        R.lane = lane;
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int nr = R.rounds();
#pragma unroll UNR
        for (int r = 0; r < (NR ? NR : nr); ++r) {
            R.fetch(r);
            const int q = NR ? r : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double g = R.v[0][q][e], g2 = R.v[1][q][e], x = R.v[2][q][e];
                const double dgg2 = g - g2, dgx = g - x, dg2x = g2 - x;
                s[0] = fma(dgg2, dgg2, s[0]);
                s[1] = fma(dgx, dgx, s[1]);
                s[2] = fma(dg2x, dg2x, s[2]);
                s[3] = fma(x, x, s[3]);
                s[4] = fma(g2, g2, s[4]);
                s[5] = fma(g, g, s[5]);
            }
        }
        wave_sum_all(s);
        double n[6], inv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            n[k] = sqrt(s[k] + a.eps);
            inv[k] = 1.0 / (n[k] * (double)a.b);
        }
        if (a.variant == 0) {
            acc_d += -n[1] + n[3] + n[0] - n[4];
            acc_g += -n[0] + n[1] + n[2];
        } else {
            const double t = (n[1] - n[3]) - (n[0] - n[5]);
            acc_g += t;
            acc_d -= t;
        }
#pragma unroll UNR
        for (int r = 0; r < (NR ? NR : nr); ++r) {
            if (!NR) R.fetch(r);           // the wide row's second pass
            const int q = NR ? r : 0;
            double o[6][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double t[6];
                head_emit(a, inv, R.v[0][q][e], R.v[1][q][e], R.v[2][q][e], t);
#pragma unroll
                for (int k = 0; k < 6; ++k) o[k][e] = t[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (a.dD[k]) store4<VEC>(a.dD[k] + off, d, r << 8, lane, o[k]);
                if (a.dGl[k]) store4<VEC>(a.dGl[k] + off, d, r << 8, lane, o[3 + k]);
            }
        }
    }
    __shared__ double red[4];
    __shared__ int last;
    const int nb = (int)gridDim.x;
    const double bd = block_sum<4>(lane == 0 ? acc_d : 0.0, red);
    const double bg = block_sum<4>(lane == 0 ? acc_g : 0.0, red);
    if (threadIdx.x < 64) {      // wave 0: publish the partials write-through, then the ticket
        if (threadIdx.x == 0) {
            store_wt(a.part + blockIdx.x, bd);
            store_wt(a.part + nb + blockIdx.x, bg);
        }
        const int l = wave_ticket(a.counter, gridDim.x);
        if (threadIdx.x == 0) last = l;
    }
    __syncthreads();
    if (!last) return;
    acquire_block();
    double td = strided_sum(a.part, (int)threadIdx.x, nb, 256);
    double tg = strided_sum(a.part + nb, (int)threadIdx.x, nb, 256);
    td = block_sum<4>(td, red);
    tg = block_sum<4>(tg, red);
    if (threadIdx.x == 0) {
        a.out[0] = (float)(td / (double)a.b);
        a.out[1] = (float)(tg / (double)a.b);
    }
    ticket_reset(a.counter);
}

// ---------------------------------------------------------------------------
// seed: U = a / n(a) - h / n(h), a = h - g; backward for an upstream W
// ---------------------------------------------------------------------------
struct SeedArgs {
    const float *H, *G, *W;
    const double *norms_in;
    float *U, *gH, *gG;
    double *norms;
    int bs, d;
    double eps;
};

template <int NR, bool VEC>
__global__ __launch_bounds__(256) void cramer_seed_fwd_kernel(SeedArgs a) {
    constexpr int UNR = NR ? NR : 1;         // rounds unrolled: all of a register-resident row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = a.d;
    for (int j = 0; j < CR_ROWS / 4; ++j) {
        const int row = blockIdx.x * CR_ROWS + 4 * j + wave;
        if (row >= a.bs) break;
        const int64_t off = (int64_t)row * d;
        RowOps<NR, VEC, 2> R;
        R.p[0] = a.H + off;
        R.p[1] = a.G + off;
        R.d = d;
        R.lane = lane;
        double s[2] = {0.0, 0.0};
        const int nr = R.rounds();
#pragma unroll UNR
        for (int r = 0; r < (NR ? NR : nr); ++r) {
            R.fetch(r);
            const int q = NR ? r : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double h = R.v[0][q][e], df = h - (double)R.v[1][q][e];
                s[0] = fma(df, df, s[0]);
                s[1] = fma(h, h, s[1]);
            }
        }
        wave_sum_all(s);
        const double na = sqrt(s[0] + a.eps), nh = sqrt(s[1] + a.eps);
        const double ia = 1.0 / na, ih = 1.0 / nh;
        if (lane == 0) {
            a.norms[2 * row] = na;
            a.norms[2 * row + 1] = nh;
        }
#pragma unroll UNR
        for (int r = 0; r < (NR ? NR : nr); ++r) {
            if (!NR) R.fetch(r);
            const int q = NR ? r : 0;
            double o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double h = R.v[0][q][e], df = h - (double)R.v[1][q][e];
                o[e] = df * ia - h * ih;
            }
            store4<VEC>(a.U + off, d, r << 8, lane, o);
        }
    }
}

// gH = P_a w - P_h w, gG = -P_a w, P_v w = (w n_v^2 - v (v.w)) / n_v^3
template <int NR, bool VEC>
__global__ __launch_bounds__(256) void cramer_seed_bwd_kernel(SeedArgs a) {
    constexpr int UNR = NR ? NR : 1;         // rounds unrolled: all of a register-resident row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = a.d;
    for (int j = 0; j < CR_ROWS / 4; ++j) {
        const int row = blockIdx.x * CR_ROWS + 4 * j + wave;
        if (row >= a.bs) break;
        const int64_t off = (int64_t)row * d;
        RowOps<NR, VEC, 3> R;
        R.p[0] = a.H + off;
        R.p[1] = a.G + off;
        R.p[2] = a.W + off;
        R.d = d;
        R.lane = lane;
        double s[2] = {0.0, 0.0};            // a.w, h.w
        const int nr = R.rounds();
#pragma unroll UNR
        for (int r = 0; r < (NR ? NR : nr); ++r) {
            R.fetch(r);
            const int q = NR ? r : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double h = R.v[0][q][e], df = h - (double)R.v[1][q][e], w = R.v[2][q][e];
                s[0] = fma(df, w, s[0]);
                s[1] = fma(h, w, s[1]);
            }
        }
        wave_sum_all(s);
        const double na = a.norms_in[2 * row], nh = a.norms_in[2 * row + 1];
        const double na2 = na * na, nh2 = nh * nh;
        const double ia3 = 1.0 / (na2 * na), ih3 = 1.0 / (nh2 * nh);
#pragma unroll UNR
        for (int r = 0; r < (NR ? NR : nr); ++r) {
            if (!NR) R.fetch(r);
            const int q = NR ? r : 0;
            double oh[4], og[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double h = R.v[0][q][e], df = h - (double)R.v[1][q][e], w = R.v[2][q][e];
                const double pa = (w * na2 - df * s[0]) * ia3;
                const double ph = (w * nh2 - h * s[1]) * ih3;
                oh[e] = pa - ph;
                og[e] = -pa;
            }
            store4<VEC>(a.gH + off, d, r << 8, lane, oh);
            store4<VEC>(a.gG + off, d, r << 8, lane, og);
        }
    }
}

inline bool cr_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int cr_blocks(int rows) { return (rows + CR_ROWS - 1) / CR_ROWS; }

// the instantiation for a width and a vector form
#define CR_DISPATCH(KERNEL, ARGS, ROWS, D, VEC, STREAM)                                        \
    do {                                                                                       \
        const dim3 grid((unsigned)cr_blocks(ROWS)), block(256);                                \
        if ((D) <= 256) {                                                                      \
            if (VEC) hipLaunchKernelGGL((KERNEL<1, true>), grid, block, 0, STREAM, ARGS);      \
            else hipLaunchKernelGGL((KERNEL<1, false>), grid, block, 0, STREAM, ARGS);         \
        } else if ((D) <= CR_REG_MAX) {                                                        \
            if (VEC) hipLaunchKernelGGL((KERNEL<4, true>), grid, block, 0, STREAM, ARGS);      \
            else hipLaunchKernelGGL((KERNEL<4, false>), grid, block, 0, STREAM, ARGS);         \
        } else {                                                                               \
            if (VEC) hipLaunchKernelGGL((KERNEL<0, true>), grid, block, 0, STREAM, ARGS);      \
            else hipLaunchKernelGGL((KERNEL<0, false>), grid, block, 0, STREAM, ARGS);         \
        }                                                                                      \
    } while (0)

}  // namespace smmd

using namespace smmd;

extern "C" {

size_t smmd_cramer_head_workspace_bytes(int b, int d) {
    if (b < 1 || d < 1) return 0;
    return CR_WS_HEADER + align_up((size_t)cr_blocks(b) * 2 * sizeof(double), 256);
}

smmd_status smmd_cramer_head_fwd(const float *G, const float *G2, const float *X, int b, int d,
                                 int variant, float eps, int want, float *out, float *dD_dG,
                                 float *dD_dG2, float *dD_dX, float *dGl_dG, float *dGl_dG2,
                                 float *dGl_dX, void *ws, size_t ws_bytes, smmd_stream_t stream) {
    if (!G || !G2 || !X || !out || b < 1 || d < 1 || !(eps >= 0.f)) return SMMD_EINVAL;
    if ((variant != 0 && variant != 1) || want < 1 || want > 3) return SMMD_EINVAL;
    if ((want & 1) && (!dD_dG || !dD_dG2 || !dD_dX)) return SMMD_EINVAL;
    if ((want & 2) && (!dGl_dG || !dGl_dG2 || !dGl_dX)) return SMMD_EINVAL;
    if (!ws || ws_bytes < smmd_cramer_head_workspace_bytes(b, d)) return SMMD_EWORKSPACE;
    HeadArgs a{};
    a.G = G;
    a.G2 = G2;
    a.X = X;
    a.out = out;
    if (want & 1) { a.dD[0] = dD_dG; a.dD[1] = dD_dG2; a.dD[2] = dD_dX; }
    if (want & 2) { a.dGl[0] = dGl_dG; a.dGl[1] = dGl_dG2; a.dGl[2] = dGl_dX; }
    a.counter = (unsigned *)ws;           // ticket first, at a fixed offset (as gp_slope_fwd)
    a.part = (double *)((char *)ws + CR_WS_HEADER);
    a.b = b;
    a.d = d;
    a.variant = variant;
    a.eps = (double)eps;
    bool vec = (d & 3) == 0 && cr_aligned16(G) && cr_aligned16(G2) && cr_aligned16(X);
    for (int k = 0; k < 3; ++k) vec = vec && cr_aligned16(a.dD[k]) && cr_aligned16(a.dGl[k]);
    CR_DISPATCH(cramer_head_kernel, a, b, d, vec, (hipStream_t)stream);
    return last_launch_status();
}

smmd_status smmd_cramer_seed_fwd(const float *H, const float *G, int bs, int d, float eps, float *U,
                                 double *norms, smmd_stream_t stream) {
    if (!H || !G || !U || !norms || bs < 1 || d < 1 || !(eps >= 0.f)) return SMMD_EINVAL;
    SeedArgs a{};
    a.H = H;
    a.G = G;
    a.U = U;
    a.norms = norms;
    a.bs = bs;
    a.d = d;
    a.eps = (double)eps;
    const bool vec = (d & 3) == 0 && cr_aligned16(H) && cr_aligned16(G) && cr_aligned16(U);
    CR_DISPATCH(cramer_seed_fwd_kernel, a, bs, d, vec, (hipStream_t)stream);
    return last_launch_status();
}

smmd_status smmd_cramer_seed_bwd(const float *H, const float *G, const double *norms,
                                 const float *W, int bs, int d, float *gH, float *gG,
                                 smmd_stream_t stream) {
    if (!H || !G || !norms || !W || !gH || !gG || bs < 1 || d < 1) return SMMD_EINVAL;
    SeedArgs a{};
    a.H = H;
    a.G = G;
    a.W = W;
    a.norms_in = norms;
    a.gH = gH;
    a.gG = gG;
    a.bs = bs;
    a.d = d;
    const bool vec = (d & 3) == 0 && cr_aligned16(H) && cr_aligned16(G) && cr_aligned16(W) &&
                     cr_aligned16(gH) && cr_aligned16(gG);
    CR_DISPATCH(cramer_seed_bwd_kernel, a, bs, d, vec, (hipStream_t)stream);
    return last_launch_status();
}

}  // extern "C"
