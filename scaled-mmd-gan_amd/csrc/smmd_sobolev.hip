// smmd_sobolev.hip -- the loss side of the Sobolev GAN baseline, gfx950
// (MI355X): the critic update's whole loss head in one launch (both energies
// of the input gradients, the constraint, the augmented-Lagrangian term and
// the next multiplier), its one-launch backward, and the weight decay over the
// optimizer's flat parameter buffer with its backward.  All fp32 in and out,
// all bandwidth- or latency-bound (a batch-64 64x64 RGB gradient is 3 MiB, the
// SNResNet critic's buffer some tens of MiB).
//
// Reference: gan/core/sobolevgan_gp.py:16-22 (the energies and the
// constraint), :29-30 (the Wasserstein head), :32-41 (the decay and the
// penalised loss), :42 (the multiplier update).
//
// Reductions are fixed-order, as in smmd_gp.hip: per-thread sums, the
// wave/block tree, one double partial per block published write-through, and
// the last block to arrive (smmd_common.hpp's ticket) sums the partials in
// index order.  Squares are formed and summed in double (the products are
// exact), so the constraint c = (e_r + e_f) / 2 - 1, a difference, is rounded
// once from sums good to double precision.  No float atomics: two runs give
// the same bits.
#include "smmd_common.hpp"

namespace smmd {

constexpr int SB_CHUNK = 4096;           // elements a block owns (16 per thread)
constexpr size_t SB_WS_HEADER = 256;     // the arrival ticket (word 0)

inline bool sb_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int64_t sb_blocks(int64_t n) { return (n + SB_CHUNK - 1) / SB_CHUNK; }

// The aligned middle [a4, b4) of [a, b): whole float4s of a 16-byte aligned
// base.  [a, a4) and [b4, b) hold at most 3 elements each.
__device__ __forceinline__ void quad_split(int64_t a, int64_t b, int64_t &a4, int64_t &b4) {
    a4 = (a + 3) & ~(int64_t)3;
    if (a4 > b) a4 = b;
    b4 = b & ~(int64_t)3;
    if (b4 < a4) b4 = a4;
}

// This thread's share of sum x[i]^2 over [a, b), in double; the block's 256
// threads together cover the range once.  vec: x is 16-byte aligned.
__device__ __forceinline__ double sq_range(const float *__restrict__ x, int64_t a, int64_t b,
                                           int vec) {
    const int t = threadIdx.x;
    double acc = 0.0;
    if (!vec) {
        for (int64_t i = a + t; i < b; i += 256) {
            const double v = (double)x[i];
            acc = fma(v, v, acc);
        }
        return acc;
    }
    int64_t a4, b4;
    quad_split(a, b, a4, b4);
    if (a + t < a4) {
        const double v = (double)x[a + t];
        acc = fma(v, v, acc);
    }
    const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
#pragma unroll 4
    for (int64_t q = (a4 >> 2) + t; q < (b4 >> 2); q += 256) {
        const float4 v = x4[q];
        const double vx = (double)v.x, vy = (double)v.y, vz = (double)v.z, vw = (double)v.w;
        acc = fma(vx, vx, acc);
        acc = fma(vy, vy, acc);
        acc = fma(vz, vz, acc);
        acc = fma(vw, vw, acc);
    }
    if (b4 + t < b) {
        const double v = (double)x[b4 + t];
        acc = fma(v, v, acc);
    }
    return acc;
}

// d[i] = k * x[i] over [a, b), the block's threads together; vec: both bases
// 16-byte aligned
__device__ __forceinline__ void scale_range(const float *__restrict__ x, float *__restrict__ d,
                                            int64_t a, int64_t b, float k, int vec) {
    const int t = threadIdx.x;
    if (!vec) {
        for (int64_t i = a + t; i < b; i += 256) d[i] = k * x[i];
        return;
    }
    int64_t a4, b4;
    quad_split(a, b, a4, b4);
    if (a + t < a4) d[a + t] = k * x[a + t];
    const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
    float4 *__restrict__ d4 = reinterpret_cast<float4 *>(d);
#pragma unroll 4
    for (int64_t q = (a4 >> 2) + t; q < (b4 >> 2); q += 256) {
        const float4 v = x4[q];
        d4[q] = make_float4(k * v.x, k * v.y, k * v.z, k * v.w);
    }
    if (b4 + t < b) d[b4 + t] = k * x[b4 + t];
}

// d[i] = 0 over [a, b) (nothing is read: whatever lies there, the result is 0)
__device__ __forceinline__ void zero_range(float *__restrict__ d, int64_t a, int64_t b, int vec) {
    const int t = threadIdx.x;
    if (!vec) {
        for (int64_t i = a + t; i < b; i += 256) d[i] = 0.f;
        return;
    }
    int64_t a4, b4;
    quad_split(a, b, a4, b4);
    if (a + t < a4) d[a + t] = 0.f;
    float4 *__restrict__ d4 = reinterpret_cast<float4 *>(d);
    for (int64_t q = (a4 >> 2) + t; q < (b4 >> 2); q += 256) d4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b4 + t < b) d[b4 + t] = 0.f;
}

// ---------------------------------------------------------------------------
// the head.  The two gradients are dense, so only their element sets matter:
// each is walked flat.  Blocks [0, nb_real) own the SB_CHUNK-element chunks of
// g_real, blocks [nb_real, nb_real + nb_fake) those of g_fake: a chunk never
// straddles the tensors, and every chunk starts on a float4 of its tensor.
// Block k publishes part[2 k] (its real sum) and part[2 k + 1] (its fake sum);
// one of the two is zero.
// ---------------------------------------------------------------------------
struct SobolevArgs {
    const float *g_real, *g_fake;    // [b_real, per], [b_fake, per], dense
    const float *d_real, *d_fake;    // forward: the critic outputs [b_real], [b_fake]
    const float *lam;                // forward: the multiplier (device scalar)
    const float *fwd;                // backward: the forward's out[6]
    const float *go;                 // backward: upstream gradient (device scalar)
    float *out;                      // forward: [6]
    float *dg_real, *dg_fake;        // backward: the inputs' layouts
    float *dd_real, *dd_fake;        // backward: [b_real], [b_fake]
    double *part;                    // forward: two partials per block
    unsigned *counter;               // forward: arrival ticket (zero at rest)
    int64_t n_real, n_fake;          // elements
    int b_real, b_fake, nb_real;
    int vec_real, vec_fake;
    float rho;
};

__global__ __launch_bounds__(256) void sobolev_fwd_kernel(SobolevArgs a) {
    const int k = blockIdx.x;
    const bool real = k < a.nb_real;
    const int64_t s = (int64_t)(real ? k : k - a.nb_real) * SB_CHUNK;
    const int64_t n = real ? a.n_real : a.n_fake;
    const int64_t e = (n - s < SB_CHUNK) ? n : s + SB_CHUNK;
    const double mine = sq_range(real ? a.g_real : a.g_fake, s, e, real ? a.vec_real : a.vec_fake);
    __shared__ double red[4];
    __shared__ int last;
    const double bs = block_sum<4>(mine, red);
    if (threadIdx.x < 64) {      // wave 0: publish the partials write-through, then the ticket
        if (threadIdx.x == 0) {
            store_wt(a.part + 2 * k, real ? bs : 0.0);
            store_wt(a.part + 2 * k + 1, real ? 0.0 : bs);
        }
        const int l = wave_ticket(a.counter, gridDim.x);
        if (threadIdx.x == 0) last = l;
    }
    __syncthreads();
    if (!last) return;
    acquire_block();
    // second level: the block partials in index order (thread-strided, then
    // the block tree), and the two critic-output sums
    const int np = 2 * (int)gridDim.x;
    double sr = strided_sum(a.part, 2 * (int)threadIdx.x, np, 512);
    double sf = strided_sum(a.part, 2 * (int)threadIdx.x + 1, np, 512);
    double mr = 0.0, mf = 0.0;
    for (int i = threadIdx.x; i < a.b_real; i += 256) mr += (double)a.d_real[i];
    for (int i = threadIdx.x; i < a.b_fake; i += 256) mf += (double)a.d_fake[i];
    sr = block_sum<4>(sr, red);
    sf = block_sum<4>(sf, red);
    mr = block_sum<4>(mr, red);
    mf = block_sum<4>(mf, red);
    if (threadIdx.x == 0) {
        const double er = sr / (double)a.b_real, ef = sf / (double)a.b_fake;
        mr /= (double)a.b_real;
        mf /= (double)a.b_fake;
        const double lam = (double)a.lam[0], rho = (double)a.rho;
        const double c = 0.5 * er + 0.5 * ef - 1.0;               // sobolevgan_gp.py:22
        a.out[0] = (float)(mf - mr + lam * c + 0.5 * rho * c * c);   // :29, :40
        a.out[1] = (float)(-mf);                                  // :30
        a.out[2] = (float)c;
        a.out[3] = (float)(lam + rho * c);                        // :42, and d out[0] / d c
        a.out[4] = (float)er;
        a.out[5] = (float)ef;
    }
    ticket_reset(a.counter);
}

// dg = go * mult / b * g per tensor over the same chunks; the critic outputs'
// gradients (constants) by the grid's first threads
__global__ __launch_bounds__(256) void sobolev_bwd_kernel(SobolevArgs a) {
    const int k = blockIdx.x;
    const bool real = k < a.nb_real;
    const int64_t s = (int64_t)(real ? k : k - a.nb_real) * SB_CHUNK;
    const int64_t n = real ? a.n_real : a.n_fake;
    const int64_t e = (n - s < SB_CHUNK) ? n : s + SB_CHUNK;
    const float go = a.go[0];
    const float kk = (go * a.fwd[3]) / (float)(real ? a.b_real : a.b_fake);
    scale_range(real ? a.g_real : a.g_fake, real ? a.dg_real : a.dg_fake, s, e, kk,
                real ? a.vec_real : a.vec_fake);
    const int64_t nth = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)k * 256 + threadIdx.x; i < (int64_t)a.b_real + a.b_fake; i += nth) {
        if (i < a.b_real) a.dd_real[i] = -go / (float)a.b_real;
        else a.dd_fake[i - a.b_real] = go / (float)a.b_fake;
    }
}

// ---------------------------------------------------------------------------
// weight decay over a flat buffer w[n].  Segment s is [off[s], off[s + 1]) of
// it with coefficient coef[s]; the table lives on the device.  Block k owns
// elements [k SB_CHUNK, (k + 1) SB_CHUNK): it finds the segment holding its
// first element by binary search and walks forward, taking from each segment
// the part inside its chunk.  Segment bounds fall anywhere (parameters are
// packed back to back): each part is walked as up to 3 leading elements, whole
// float4s, up to 3 trailing ones.  Every position of a chunk is visited once
// whatever the table holds, and no index leaves the chunk: a table that is not
// ascending gives wrong values, never a wild access.
// ---------------------------------------------------------------------------
struct DecayArgs {
    const float *w;
    const int64_t *off;          // [nseg + 1], device
    const float *coef;           // [nseg], device
    const float *go;             // backward: upstream gradient (device scalar)
    float *out;                  // forward: [1]
    float *dw;                   // backward: [n]
    double *part;                // forward: one partial per block
    unsigned *counter;           // forward: arrival ticket (zero at rest)
    int64_t n;
    int nseg, vec;
};

// the last segment whose start is <= s (0 when s lies before the table)
__device__ __forceinline__ int decay_first_segment(const int64_t *__restrict__ off, int nseg,
                                                   int64_t s) {
    int lo = 0, hi = nseg;       // first j in [0, nseg] with off[j] > s
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] > s) hi = mid; else lo = mid + 1;
    }
    return lo > 0 ? lo - 1 : 0;
}

__device__ __forceinline__ int64_t clamp64(int64_t x, int64_t lo, int64_t hi) {
    return x < lo ? lo : (x > hi ? hi : x);
}

__global__ __launch_bounds__(256) void decay_fwd_kernel(DecayArgs a) {
    const int64_t s = (int64_t)blockIdx.x * SB_CHUNK;
    const int64_t e = (a.n - s < SB_CHUNK) ? a.n : s + SB_CHUNK;
    double acc = 0.0;
    int64_t pos = s;
    for (int seg = decay_first_segment(a.off, a.nseg, s); seg < a.nseg && pos < e; ++seg) {
        const int64_t lo = clamp64(a.off[seg], pos, e), hi = clamp64(a.off[seg + 1], lo, e);
        const float cf = a.coef[seg];
        // the segment's sum scaled in double before it joins the partial
        if (hi > lo && cf != 0.f) acc += (double)cf * sq_range(a.w, lo, hi, a.vec);
        pos = hi;
    }
    __shared__ double red[4];
    __shared__ int last;
    const double bs = block_sum<4>(acc, red);
    if (threadIdx.x < 64) {
        if (threadIdx.x == 0) store_wt(a.part + blockIdx.x, bs);
        const int l = wave_ticket(a.counter, gridDim.x);
        if (threadIdx.x == 0) last = l;
    }
    __syncthreads();
    if (!last) return;
    acquire_block();
    double t = strided_sum(a.part, (int)threadIdx.x, (int)gridDim.x, 256);
    t = block_sum<4>(t, red);
    if (threadIdx.x == 0) a.out[0] = (float)t;
    ticket_reset(a.counter);
}

// dw = go * 2 coef_s * w inside segment s, 0 outside every segment and inside
// one whose coefficient is 0 (written without reading w)
__global__ __launch_bounds__(256) void decay_bwd_kernel(DecayArgs a) {
    const int64_t s = (int64_t)blockIdx.x * SB_CHUNK;
    const int64_t e = (a.n - s < SB_CHUNK) ? a.n : s + SB_CHUNK;
    const float g2 = a.go[0] * 2.f;
    int64_t pos = s;
    for (int seg = decay_first_segment(a.off, a.nseg, s); seg < a.nseg && pos < e; ++seg) {
        const int64_t lo = clamp64(a.off[seg], pos, e), hi = clamp64(a.off[seg + 1], lo, e);
        const float cf = a.coef[seg];
        zero_range(a.dw, pos, lo, a.vec);
        if (cf != 0.f) scale_range(a.w, a.dw, lo, hi, g2 * cf, a.vec);
        else zero_range(a.dw, lo, hi, a.vec);
        pos = hi;
    }
    zero_range(a.dw, pos, e, a.vec);
}

inline bool sobolev_grid(int b_real, int b_fake, int64_t per, int64_t &nbr, int64_t &nbf) {
    if (b_real < 1 || b_fake < 1 || per < 1) return false;
    // (both element counts under 2^39: the block count and twice it fit an int)
    if (per > ((int64_t)1 << 39) / (b_real > b_fake ? b_real : b_fake)) return false;
    nbr = sb_blocks((int64_t)b_real * per);
    nbf = sb_blocks((int64_t)b_fake * per);
    return true;
}

}  // namespace smmd

using namespace smmd;

extern "C" {

size_t smmd_sobolev_workspace_bytes(int b_real, int b_fake, int64_t per) {
    int64_t nbr, nbf;
    if (!sobolev_grid(b_real, b_fake, per, nbr, nbf)) return 0;
    return SB_WS_HEADER + align_up((size_t)(nbr + nbf) * 2 * sizeof(double), 256);
}

smmd_status smmd_sobolev_fwd(const float *g_real, const float *g_fake, const float *d_real,
                             const float *d_fake, int b_real, int b_fake, int64_t per,
                             const float *lam, float rho, float *out, void *ws, size_t ws_bytes,
                             smmd_stream_t stream) {
    if (!g_real || !g_fake || !d_real || !d_fake || !lam || !out || !(rho >= 0.f))
        return SMMD_EINVAL;
    int64_t nbr, nbf;
    if (!sobolev_grid(b_real, b_fake, per, nbr, nbf)) return SMMD_EINVAL;
    if (!ws || ws_bytes < smmd_sobolev_workspace_bytes(b_real, b_fake, per)) return SMMD_EWORKSPACE;
    SobolevArgs a{};
    a.g_real = g_real;
    a.g_fake = g_fake;
    a.d_real = d_real;
    a.d_fake = d_fake;
    a.lam = lam;
    a.out = out;
    a.counter = (unsigned *)ws;          // ticket first, at a fixed offset (as smmd_gp_slope_fwd)
    a.part = (double *)((char *)ws + SB_WS_HEADER);
    a.n_real = (int64_t)b_real * per;
    a.n_fake = (int64_t)b_fake * per;
    a.b_real = b_real;
    a.b_fake = b_fake;
    a.nb_real = (int)nbr;
    a.vec_real = sb_aligned16(g_real);
    a.vec_fake = sb_aligned16(g_fake);
    a.rho = rho;
    hipLaunchKernelGGL(sobolev_fwd_kernel, dim3((unsigned)(nbr + nbf)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return last_launch_status();
}

smmd_status smmd_sobolev_bwd(const float *g_real, const float *g_fake, int b_real, int b_fake,
                             int64_t per, const float *fwd_out, const float *go, float *dg_real,
                             float *dg_fake, float *dd_real, float *dd_fake,
                             smmd_stream_t stream) {
    if (!g_real || !g_fake || !fwd_out || !go || !dg_real || !dg_fake || !dd_real || !dd_fake)
        return SMMD_EINVAL;
    int64_t nbr, nbf;
    if (!sobolev_grid(b_real, b_fake, per, nbr, nbf)) return SMMD_EINVAL;
    SobolevArgs a{};
    a.g_real = g_real;
    a.g_fake = g_fake;
    a.fwd = fwd_out;
    a.go = go;
    a.dg_real = dg_real;
    a.dg_fake = dg_fake;
    a.dd_real = dd_real;
    a.dd_fake = dd_fake;
    a.n_real = (int64_t)b_real * per;
    a.n_fake = (int64_t)b_fake * per;
    a.b_real = b_real;
    a.b_fake = b_fake;
    a.nb_real = (int)nbr;
    a.vec_real = sb_aligned16(g_real) && sb_aligned16(dg_real);
    a.vec_fake = sb_aligned16(g_fake) && sb_aligned16(dg_fake);
    hipLaunchKernelGGL(sobolev_bwd_kernel, dim3((unsigned)(nbr + nbf)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return last_launch_status();
}

size_t smmd_decay_workspace_bytes(int64_t n) {
    if (n < 1 || sb_blocks(n) > 0x7fffffff / 2) return 0;
    return SB_WS_HEADER + align_up((size_t)sb_blocks(n) * sizeof(double), 256);
}

smmd_status smmd_decay_fwd(const float *flat, int64_t n, const int64_t *offsets,
                           const float *coefs, int nseg, float *out, void *ws, size_t ws_bytes,
                           smmd_stream_t stream) {
    if (!flat || !offsets || !coefs || !out || n < 1 || nseg < 1) return SMMD_EINVAL;
    if (sb_blocks(n) > 0x7fffffff / 2) return SMMD_EINVAL;
    if (!ws || ws_bytes < smmd_decay_workspace_bytes(n)) return SMMD_EWORKSPACE;
    DecayArgs a{};
    a.w = flat;
    a.off = offsets;
    a.coef = coefs;
    a.out = out;
    a.counter = (unsigned *)ws;
    a.part = (double *)((char *)ws + SB_WS_HEADER);
    a.n = n;
    a.nseg = nseg;
    a.vec = sb_aligned16(flat);
    hipLaunchKernelGGL(decay_fwd_kernel, dim3((unsigned)sb_blocks(n)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return last_launch_status();
}

smmd_status smmd_decay_bwd(const float *flat, int64_t n, const int64_t *offsets,
                           const float *coefs, int nseg, const float *go, float *dflat,
                           smmd_stream_t stream) {
    if (!flat || !offsets || !coefs || !go || !dflat || n < 1 || nseg < 1) return SMMD_EINVAL;
    if (sb_blocks(n) > 0x7fffffff / 2) return SMMD_EINVAL;
    DecayArgs a{};
    a.w = flat;
    a.off = offsets;
    a.coef = coefs;
    a.go = go;
    a.dw = dflat;
    a.n = n;
    a.nseg = nseg;
    a.vec = sb_aligned16(flat) && sb_aligned16(dflat);
    hipLaunchKernelGGL(decay_bwd_kernel, dim3((unsigned)sb_blocks(n)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return last_launch_status();
}

}  // extern "C"
