// smmd_gp.hip -- the loss side of the GAN and WGAN-GP baselines, gfx950
// (MI355X): the gradient penalty's interpolates, its per-pixel slopes with
// their penalty and backward, and the one-launch critic head.  All fp32, all
// bandwidth- or latency-bound (the largest operand, a batch-64 64x64 RGB
// gradient, is 3 MiB).
//
// Reference: gan/core/wgan_gp.py:10-25 (interpolates, slopes, penalty, the
// Wasserstein head), gan/core/gan.py:10-11 (the softplus head),
// gan/core/cramer.py:78 and gan/core/model.py:330-343 (the (1-a) x + a y form
// of the interpolates and safer_norm's eps, for later adopters).
//
// Reductions are fixed-order: per-thread sums, the wave/block tree, one double
// partial per block published write-through, and the last block to arrive
// (smmd_common.hpp's ticket) sums the partials in index order.  No float
// atomics: two runs give the same bits.
#include "smmd_common.hpp"

namespace smmd {

// ---------------------------------------------------------------------------
// interpolates: out[i, :] = real[i, :] + alpha[i] (fake[i, :] - real[i, :])
// (form 0) or (1 - alpha[i]) real[i, :] + alpha[i] fake[i, :] (form 1) over
// b dense rows of `per` floats.  The three tensors are dense, so the flat
// buffer is walked as float4 whatever `per` is; when per % 4 != 0 a float4
// straddles rows and each of its elements looks its own row's alpha up.
// Every operation rounds on its own (no contraction): the result has the
// bits of the same expression in separate tensor ops.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float interp_one(float r, float f, float a, int form) {
#pragma clang fp contract(off)
    if (form == 0) {
        const float d = f - r;
        const float t = a * d;
        return r + t;
    }
    const float w = 1.f - a;
    const float x = w * r;
    const float y = a * f;
    return x + y;
}

__global__ __launch_bounds__(256) void gp_interp_kernel(const float *__restrict__ real,
                                                        const float *__restrict__ fake,
                                                        const float *__restrict__ alpha,
                                                        float *__restrict__ out, int64_t total,
                                                        int64_t per, int form, int vec) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * 256;
    if (!vec) {          // a base off 16 bytes (a view with a storage offset)
        for (int64_t i = tid; i < total; i += nth)
            out[i] = interp_one(real[i], fake[i], alpha[i / per], form);
        return;
    }
    const int64_t n4 = total >> 2;
    for (int64_t i = tid; i < n4; i += nth) {
        const float4 r = reinterpret_cast<const float4 *>(real)[i];
        const float4 f = reinterpret_cast<const float4 *>(fake)[i];
        const int64_t e = i << 2;
        int64_t row = e / per;
        float4 o;
        if ((per & 3) == 0) {        // the float4 lies in one row
            const float a = alpha[row];
            o.x = interp_one(r.x, f.x, a, form);
            o.y = interp_one(r.y, f.y, a, form);
            o.z = interp_one(r.z, f.z, a, form);
            o.w = interp_one(r.w, f.w, a, form);
        } else {
            int64_t rem = e - row * per;     // position inside the row
            const float rr[4] = {r.x, r.y, r.z, r.w}, ff[4] = {f.x, f.y, f.z, f.w};
            float oo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                oo[j] = interp_one(rr[j], ff[j], alpha[row], form);
                if (++rem == per) { rem = 0; ++row; }
            }
            o = make_float4(oo[0], oo[1], oo[2], oo[3]);
        }
        reinterpret_cast<float4 *>(out)[i] = o;
    }
    // the tail past the last whole float4 (total % 4 elements)
    const int64_t i = (n4 << 2) + tid;
    if (i < total) out[i] = interp_one(real[i], fake[i], alpha[i / per], form);
}

// ---------------------------------------------------------------------------
// slopes.  Pixel p = (sample, y, x) in that order, n = b * hw of them; block k
// owns pixels [k * SL_CHUNK, (k + 1) * SL_CHUNK), thread t the four
// consecutive pixels from k * SL_CHUNK + 4 t.
//   NCHW: element (p, ch) at ((p / hw) * c + ch) * hw + p % hw: with
//         hw % 4 == 0 a thread's four pixels are one float4 per channel.
//   channels-last: element (p, ch) at p * c + ch: a thread's four pixels are
//         4 c contiguous floats, c float4s.
// `vec`: those float4 forms are aligned (bases 16-byte aligned; NCHW:
// hw % 4 == 0); a group cut by the end of the tensor, or any group without
// `vec`, goes element by element.  Channel sums run in channel order.
// ---------------------------------------------------------------------------
constexpr int SL_CHUNK = 1024;
constexpr size_t SL_WS_HEADER = 256;     // the arrival ticket (word 0)

struct SlopeArgs {
    const float *g;          // the input gradient
    const float *slopes_in;  // backward: the forward's slopes
    const float *go;         // backward: upstream gradient (device scalar)
    float *slopes;           // forward: [n]
    float *out;              // forward: [1] penalty
    float *dg;               // backward: g's layout
    double *part;            // forward: one partial per block
    unsigned *counter;       // forward: arrival ticket (zero at rest)
    int64_t n;               // pixels
    int c, hw, channels_last, vec;
    float eps;
};

// sum over channels of g^2 for the thread's (up to) four pixels from p0
__device__ __forceinline__ void slope_sq4(const SlopeArgs &a, int64_t p0, int cnt, float (&ss)[4]) {
    const float *__restrict__ g = a.g;
    const int c = a.c, hw = a.hw;
    ss[0] = ss[1] = ss[2] = ss[3] = 0.f;
    if (a.vec && cnt == 4) {
        if (a.channels_last) {
            const float4 *q = reinterpret_cast<const float4 *>(g + p0 * c);
            int pix = 0, rem = 0;
            for (int k = 0; k < c; ++k) {
                const float4 v = q[k];
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sq = e[j] * e[j];
                    ss[0] += (pix == 0) ? sq : 0.f;
                    ss[1] += (pix == 1) ? sq : 0.f;
                    ss[2] += (pix == 2) ? sq : 0.f;
                    ss[3] += (pix == 3) ? sq : 0.f;
                    if (++rem == c) { rem = 0; ++pix; }
                }
            }
        } else {
            const int64_t s = p0 / hw;
            const float *base = g + (s * c) * hw + (p0 - s * hw);
            for (int ch = 0; ch < c; ++ch) {
                const float4 v = *reinterpret_cast<const float4 *>(base + (int64_t)ch * hw);
                ss[0] = fmaf(v.x, v.x, ss[0]);
                ss[1] = fmaf(v.y, v.y, ss[1]);
                ss[2] = fmaf(v.z, v.z, ss[2]);
                ss[3] = fmaf(v.w, v.w, ss[3]);
            }
        }
        return;
    }
    for (int j = 0; j < cnt; ++j) {
        const int64_t p = p0 + j;
        const int64_t s = p / hw;
        const float *q = a.channels_last ? g + p * c : g + (s * c) * hw + (p - s * hw);
        const int64_t step = a.channels_last ? 1 : hw;
        float acc = 0.f;
        for (int ch = 0; ch < c; ++ch) {
            const float v = q[ch * step];
            acc = fmaf(v, v, acc);
        }
        ss[j] = acc;
    }
}

__global__ __launch_bounds__(256) void gp_slope_fwd_kernel(SlopeArgs a) {
    const int64_t p0 = (int64_t)blockIdx.x * SL_CHUNK + threadIdx.x * 4;
    float pen = 0.f;
    if (p0 < a.n) {
        const int cnt = (a.n - p0 < 4) ? (int)(a.n - p0) : 4;
        float ss[4];
        slope_sq4(a, p0, cnt, ss);
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = sqrtf(ss[j] + a.eps);
            const float d = s[j] - 1.f;
            if (j < cnt) pen = fmaf(d, d, pen);
        }
        if (a.vec && cnt == 4) {
            *reinterpret_cast<float4 *>(a.slopes + p0) = make_float4(s[0], s[1], s[2], s[3]);
        } else {
            for (int j = 0; j < cnt; ++j) a.slopes[p0 + j] = s[j];
        }
    }
    __shared__ double red[4];
    __shared__ int last;
    const double bs = block_sum<4>((double)pen, red);
    if (threadIdx.x < 64) {      // wave 0: publish the partial write-through, then the ticket
        if (threadIdx.x == 0) store_wt(a.part + blockIdx.x, bs);
        const int l = wave_ticket(a.counter, gridDim.x);
        if (threadIdx.x == 0) last = l;
    }
    __syncthreads();
    if (!last) return;
    acquire_block();
    // second level: the block partials in index order (thread-strided, then
    // the block tree)
    double t = strided_sum(a.part, (int)threadIdx.x, (int)gridDim.x, 256);
    t = block_sum<4>(t, red);
    if (threadIdx.x == 0) a.out[0] = (float)(t / (double)a.n);
    ticket_reset(a.counter);
}

// dg = go * 2 (s - 1) / (s n) * g, in g's layout
__global__ __launch_bounds__(256) void gp_slope_bwd_kernel(SlopeArgs a) {
    const int64_t p0 = (int64_t)blockIdx.x * SL_CHUNK + threadIdx.x * 4;
    if (p0 >= a.n) return;
    const int cnt = (a.n - p0 < 4) ? (int)(a.n - p0) : 4;
    const float k0 = a.go[0] * (2.f / (float)a.n);
    const float *__restrict__ g = a.g;
    float *__restrict__ dg = a.dg;
    const int c = a.c, hw = a.hw;
    float cf[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec && cnt == 4) {
        const float4 s = *reinterpret_cast<const float4 *>(a.slopes_in + p0);
        cf[0] = k0 * ((s.x - 1.f) / s.x);
        cf[1] = k0 * ((s.y - 1.f) / s.y);
        cf[2] = k0 * ((s.z - 1.f) / s.z);
        cf[3] = k0 * ((s.w - 1.f) / s.w);
        if (a.channels_last) {
            const float4 *q = reinterpret_cast<const float4 *>(g + p0 * c);
            float4 *o = reinterpret_cast<float4 *>(dg + p0 * c);
            int pix = 0, rem = 0;
            for (int k = 0; k < c; ++k) {
                const float4 v = q[k];
                const float e[4] = {v.x, v.y, v.z, v.w};
                float r[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float f = pix == 0 ? cf[0] : pix == 1 ? cf[1] : pix == 2 ? cf[2] : cf[3];
                    r[j] = f * e[j];
                    if (++rem == c) { rem = 0; ++pix; }
                }
                o[k] = make_float4(r[0], r[1], r[2], r[3]);
            }
        } else {
            const int64_t sm = p0 / hw;
            const int64_t off = (sm * c) * hw + (p0 - sm * hw);
            for (int ch = 0; ch < c; ++ch) {
                const float4 v = *reinterpret_cast<const float4 *>(g + off + (int64_t)ch * hw);
                *reinterpret_cast<float4 *>(dg + off + (int64_t)ch * hw) =
                    make_float4(cf[0] * v.x, cf[1] * v.y, cf[2] * v.z, cf[3] * v.w);
            }
        }
        return;
    }
    for (int j = 0; j < cnt; ++j) {
        const int64_t p = p0 + j;
        const float s = a.slopes_in[p];
        const float f = k0 * ((s - 1.f) / s);
        const int64_t sm = p / hw;
        const int64_t off = a.channels_last ? p * c : (sm * c) * hw + (p - sm * hw);
        const int64_t step = a.channels_last ? 1 : hw;
        for (int ch = 0; ch < c; ++ch) dg[off + ch * step] = f * g[off + ch * step];
    }
}

inline int64_t slope_blocks(int64_t n) { return (n + SL_CHUNK - 1) / SL_CHUNK; }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------
// critic head: one 256-thread block.  softplus(x) = max(x, 0) + log1p(e),
// sigmoid(x) = 1 / (1 + e) for x >= 0 and e / (1 + e) below, e = exp(-|x|):
// neither overflows, and softplus(100) is 100.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float x, float e) { return fmaxf(x, 0.f) + log1pf(e); }

__device__ __forceinline__ float sigmoid_f(float x, float e) {
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

__global__ __launch_bounds__(256) void critic_head_kernel(const float *__restrict__ d_real,
                                                          int n_real,
                                                          const float *__restrict__ d_fake,
                                                          int n_fake, int kind,
                                                          float *__restrict__ out,
                                                          float *__restrict__ g_real,
                                                          float *__restrict__ g_fake,
                                                          float *__restrict__ gg_fake) {
    __shared__ double red[4];
    const float ir = 1.f / (float)n_real, jf = 1.f / (float)n_fake;
    double sr = 0.0, sf = 0.0, sg = 0.0;     // sums behind out[0] (real, fake) and out[1]
    for (int i = threadIdx.x; i < n_real; i += 256) {
        const float x = d_real[i];
        if (kind == 0) {
            sr += (double)x;
            g_real[i] = -ir;
        } else {
            const float e = expf(-fabsf(x));
            sr += (double)softplus_f(-x, e);            // gan.py:10
            g_real[i] = -sigmoid_f(-x, e) * ir;
        }
    }
    for (int i = threadIdx.x; i < n_fake; i += 256) {
        const float x = d_fake[i];
        if (kind == 0) {
            sf += (double)x;
            g_fake[i] = jf;
            gg_fake[i] = -jf;
        } else {
            const float e = expf(-fabsf(x));
            sf += (double)softplus_f(x, e);             // gan.py:10
            sg += (double)softplus_f(-x, e);            // gan.py:11
            g_fake[i] = sigmoid_f(x, e) * jf;
            gg_fake[i] = -sigmoid_f(-x, e) * jf;
        }
    }
    sr = block_sum<4>(sr, red);
    sf = block_sum<4>(sf, red);
    sg = block_sum<4>(sg, red);
    if (threadIdx.x == 0) {
        const double mr = sr / (double)n_real, mf = sf / (double)n_fake;
        if (kind == 0) {
            out[0] = (float)(mf - mr);                  // wgan_gp.py:24
            out[1] = (float)(-mf);                      // wgan_gp.py:25
        } else {
            out[0] = (float)(mr + mf);
            out[1] = (float)(sg / (double)n_fake);
        }
    }
}

}  // namespace smmd

using namespace smmd;

extern "C" {

smmd_status smmd_gp_interp(const float *real, const float *fake, const float *alpha, float *out,
                           int b, int64_t per, int form, smmd_stream_t stream) {
    if (!real || !fake || !alpha || !out || b < 1 || per < 1) return SMMD_EINVAL;
    if (form != 0 && form != 1) return SMMD_EINVAL;
    const int64_t total = (int64_t)b * per;
    const int vec = aligned16(real) && aligned16(fake) && aligned16(out);
    int64_t blocks = ((vec ? (total + 3) / 4 : total) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(gp_interp_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       real, fake, alpha, out, total, per, form, vec);
    return last_launch_status();
}

size_t smmd_gp_slope_workspace_bytes(int b, int c, int hw) {
    if (b < 1 || c < 1 || hw < 1) return 0;
    return SL_WS_HEADER + align_up((size_t)slope_blocks((int64_t)b * hw) * sizeof(double), 256);
}

smmd_status smmd_gp_slope_fwd(const float *g, int b, int c, int hw, int channels_last, float eps,
                              float *out, float *slopes, void *ws, size_t ws_bytes,
                              smmd_stream_t stream) {
    if (!g || !out || !slopes || b < 1 || c < 1 || hw < 1 || !(eps >= 0.f)) return SMMD_EINVAL;
    const int64_t n = (int64_t)b * hw;
    const int64_t blocks = slope_blocks(n);
    if (blocks > 0x7fffffff / 2) return SMMD_EINVAL;
    if (!ws || ws_bytes < smmd_gp_slope_workspace_bytes(b, c, hw)) return SMMD_EWORKSPACE;
    SlopeArgs a{};
    a.g = g;
    a.slopes = slopes;
    a.out = out;
    // ticket first, at a fixed offset: a cached workspace reused for a smaller
    // call must not find its counter inside an earlier call's partials
    a.counter = (unsigned *)ws;
    a.part = (double *)((char *)ws + SL_WS_HEADER);
    a.n = n;
    a.c = c;
    a.hw = hw;
    a.channels_last = channels_last ? 1 : 0;
    a.vec = aligned16(g) && aligned16(slopes) && (channels_last || (hw & 3) == 0);
    a.eps = eps;
    hipLaunchKernelGGL(gp_slope_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, a);
    return last_launch_status();
}

smmd_status smmd_gp_slope_bwd(const float *g, const float *slopes, int b, int c, int hw,
                              int channels_last, const float *go, float *dg,
                              smmd_stream_t stream) {
    if (!g || !slopes || !go || !dg || b < 1 || c < 1 || hw < 1) return SMMD_EINVAL;
    const int64_t n = (int64_t)b * hw;
    const int64_t blocks = slope_blocks(n);
    if (blocks > 0x7fffffff / 2) return SMMD_EINVAL;
    SlopeArgs a{};
    a.g = g;
    a.slopes_in = slopes;
    a.go = go;
    a.dg = dg;
    a.n = n;
    a.c = c;
    a.hw = hw;
    a.channels_last = channels_last ? 1 : 0;
    a.vec = aligned16(g) && aligned16(dg) && aligned16(slopes) &&
            (channels_last || (hw & 3) == 0);
    hipLaunchKernelGGL(gp_slope_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, a);
    return last_launch_status();
}

smmd_status smmd_critic_head_fwd(const float *d_real, int n_real, const float *d_fake, int n_fake,
                                 int kind, float *out, float *g_real, float *g_fake,
                                 float *gg_fake, smmd_stream_t stream) {
    if (!d_real || !d_fake || !out || !g_real || !g_fake || !gg_fake) return SMMD_EINVAL;
    if (n_real < 1 || n_fake < 1 || (kind != 0 && kind != 1)) return SMMD_EINVAL;
    hipLaunchKernelGGL(critic_head_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_real,
                       n_real, d_fake, n_fake, kind, out, g_real, g_fake, gg_fake);
    return last_launch_status();
}

}  // extern "C"
