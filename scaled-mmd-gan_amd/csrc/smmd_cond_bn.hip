// smmd_cond_bn.hip -- class-conditional batch norm + ReLU of the conditional
// generator's up blocks (gfx950 / MI355X): the forward, with or without the
// record its backward needs, and that backward (the generator step).
//
// Reference: resnet/ops/cond_batchnorm.py:6-17 (tf.nn.moments over (N, H, W),
// tf.nn.batch_normalization with eps 1e-5 and the rows labels[n] of the
// [num_classes, C] offset / scale tables; no moving averages) then tf.nn.relu
// (resnet/block.py:42-47):
//   z[n, c, :] = (x - mean_c) inv_c scale[l_n, c] + offset[l_n, c],  y = relu(z)
//
// The forward is the two launches of smmd_bnrelu.hip over [N, C, HW] NCHW
// fp32 on the grid (C, S): its statistics pass unchanged (bn_stats_kernel,
// shifted sums, block tree in double, a [S][C] slab), then an apply pass whose
// scale and shift are looked up per sample.  A label outside [0, num_classes)
// is clamped into the tables.  HBM: one read for the statistics, one read +
// one write to apply.
#include "smmd_bn_stats.hpp"

namespace smmd {

__device__ __forceinline__ int cbn_label(const int *__restrict__ labels, int n, int K) {
    return min(max(labels[n], 0), K - 1);
}

// The lanes of a row: thread t works on row slot r, column col of its rows
// (rpi row slots per step on maps shorter than the block, as bn_stats_kernel).
struct CbnLane {
    int w4, rpi, r, col, step;
    __device__ __forceinline__ explicit CbnLane(int HW) {
        w4 = HW >> 2;
        rpi = w4 >= BN_T ? 1 : BN_T / w4;
        r = w4 >= BN_T ? 0 : (int)threadIdx.x / w4;
        col = w4 >= BN_T ? (int)threadIdx.x : (int)threadIdx.x - r * w4;
        step = w4 >= BN_T ? BN_T : w4;
    }
};

__global__ __launch_bounds__(BN_T) void cond_bn_apply_kernel(
    const float *__restrict__ x, const int *__restrict__ labels, int N, int C, int HW, int S, int K,
    const double *__restrict__ part, const float *__restrict__ scale,
    const float *__restrict__ offset, float eps, float *__restrict__ y, float *__restrict__ save) {
    const int c = blockIdx.x, s = blockIdx.y;
    __shared__ float sh[3];
    if (threadIdx.x < SMMD_WAVE) {
        // fixed order: lane-strided over the S partials, then the wave tree
        double a = 0.0, q = 0.0;
        for (int j = threadIdx.x; j < S; j += SMMD_WAVE) {
            a += part[((size_t)j * C + c) * 2 + 0];
            q += part[((size_t)j * C + c) * 2 + 1];
        }
        a = wave_sum(a);
        q = wave_sum(q);
        if (threadIdx.x == 0) {
            const double cnt = (double)N * (double)HW;
            const double ms = a / cnt;                   // mean of x - k
            double var = q / cnt - ms * ms;
            if (var < 0.0) var = 0.0;
            sh[0] = x[(size_t)c * HW];                  // the shift k
            sh[1] = (float)ms;                           // mean - k
            sh[2] = (float)(1.0 / sqrt(var + (double)eps));
            if (s == 0 && save) {                        // for smmd_cond_bn_relu_bwd
                save[3 * c + 0] = sh[0];
                save[3 * c + 1] = sh[1];
                save[3 * c + 2] = sh[2];
            }
        }
    }
    __syncthreads();
    const float k = sh[0], ms = sh[1], inv = sh[2];
    int n0, n1;
    bn_rows(N, S, s, n0, n1);
    const CbnLane ln(HW);
    if (ln.r >= ln.rpi) return;
    for (int n = n0 + ln.r; n < n1; n += ln.rpi) {
        const size_t t = (size_t)cbn_label(labels, n, K) * C + c;
        // z = ((x - k) - (mean - k)) * (scale inv) + offset: the backward forms
        // the same float operations from save, so its ReLU mask is this one
        const float sc = scale[t] * inv, bb = offset[t];
        const size_t off = ((size_t)n * C + c) * HW;
        const float4 *row = reinterpret_cast<const float4 *>(x + off);
        float4 *out = reinterpret_cast<float4 *>(y + off);
        for (int i = ln.col; i < ln.w4; i += ln.step) {
            const float4 v = row[i];
            out[i] = make_float4(fmaxf(fmaf((v.x - k) - ms, sc, bb), 0.f),
                                 fmaxf(fmaf((v.y - k) - ms, sc, bb), 0.f),
                                 fmaxf(fmaf((v.z - k) - ms, sc, bb), 0.f),
                                 fmaxf(fmaf((v.w - k) - ms, sc, bb), 0.f));
        }
    }
}

// ---- backward ----------------------------------------------------------------
// With gz = gy [z > 0] (z as the forward formed it), xhat = (x - mean) inv,
// gamma[n, c] = scale[l_n, c], M = N HW:
//   a[n, c] = sum_hw gz,  b[n, c] = sum_hw gz xhat
//   goffset[k, c] = sum_{n: l_n = k} a[n, c],  gscale[k, c] the same over b
//   S1_c = sum_n gamma a,  S2_c = sum_n gamma b
//   gx = inv (gamma gz - S1 / M - xhat S2 / M)
// Pass 1 (grid (C, S)): a, b per sample and channel in double (each row's
// lanes summed by a fixed tree in LDS) to ab[N][C][2].  A table launch (one
// thread per table entry) sums ab over the samples of each class in sample
// order; it writes every entry, zero for an absent class.  Pass 2 (grid (C, S)):
// every block sums S1, S2 of its channel over the samples in a fixed order and
// writes gx.  HBM: x, gy read twice, gx written once, as the unconditional pair.
__device__ __forceinline__ void cbn_bwd_elem(float x, float g, float k, float ms, float inv,
                                             float sc, float bb, float &gz, float &xh) {
    const float xm = (x - k) - ms;
    gz = (fmaf(xm, sc, bb) > 0.f) ? g : 0.f;
    xh = xm * inv;
}

__global__ __launch_bounds__(BN_T) void cond_bn_bwd_rows_kernel(
    const float *__restrict__ x, const float *__restrict__ gy, const int *__restrict__ labels, int N,
    int C, int HW, int S, int K, const float *__restrict__ scale, const float *__restrict__ offset,
    const float *__restrict__ save, double *__restrict__ ab) {
    const int c = blockIdx.x, s = blockIdx.y;
    int n0, n1;
    bn_rows(N, S, s, n0, n1);
    const CbnLane ln(HW);
    const float k = save[3 * c + 0], ms = save[3 * c + 1], inv = save[3 * c + 2];
    __shared__ double sa[BN_T], sb[BN_T];
    const int t = threadIdx.x;
    // every thread takes every step of the loop (the barriers); the row slots
    // past the block's rows and the lanes past the last whole row carry zeros
    for (int nb = n0; nb < n1; nb += ln.rpi) {
        const int n = nb + ln.r;
        const bool on = ln.r < ln.rpi && n < n1;
        float a = 0.f, q = 0.f;
        if (on) {
            const size_t e = (size_t)cbn_label(labels, n, K) * C + c;
            const float sc = scale[e] * inv, bb = offset[e];
            const size_t off = ((size_t)n * C + c) * HW;
            const float4 *xr = reinterpret_cast<const float4 *>(x + off);
            const float4 *gr = reinterpret_cast<const float4 *>(gy + off);
            for (int i = ln.col; i < ln.w4; i += ln.step) {
                const float4 v = xr[i], g = gr[i];
                float gz, xh;
                cbn_bwd_elem(v.x, g.x, k, ms, inv, sc, bb, gz, xh); a += gz; q = fmaf(gz, xh, q);
                cbn_bwd_elem(v.y, g.y, k, ms, inv, sc, bb, gz, xh); a += gz; q = fmaf(gz, xh, q);
                cbn_bwd_elem(v.z, g.z, k, ms, inv, sc, bb, gz, xh); a += gz; q = fmaf(gz, xh, q);
                cbn_bwd_elem(v.w, g.w, k, ms, inv, sc, bb, gz, xh); a += gz; q = fmaf(gz, xh, q);
            }
        }
        sa[t] = (double)a;
        sb[t] = (double)q;
        __syncthreads();
        // the row's ln.step lanes (t - col .. t - col + step - 1, all inside
        // the block) summed by halving: lane col adds lane col + half
        for (int w = ln.step; w > 1;) {
            const int half = (w + 1) >> 1;
            if (on && ln.col < w - half) {
                sa[t] += sa[t + half];
                sb[t] += sb[t + half];
            }
            __syncthreads();
            w = half;
        }
        if (on && ln.col == 0) {
            ab[((size_t)n * C + c) * 2 + 0] = sa[t];
            ab[((size_t)n * C + c) * 2 + 1] = sb[t];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BN_T) void cond_bn_table_kernel(const double *__restrict__ ab,
                                                             const int *__restrict__ labels, int N,
                                                             int C, int K,
                                                             float *__restrict__ gscale,
                                                             float *__restrict__ goffset) {
    const int k = blockIdx.x;
    const int c = blockIdx.y * BN_T + (int)threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int n = 0; n < N; ++n) {                        // sample order
        if (cbn_label(labels, n, K) != k) continue;      // uniform over the block
        a += ab[((size_t)n * C + c) * 2 + 0];
        b += ab[((size_t)n * C + c) * 2 + 1];
    }
    goffset[(size_t)k * C + c] = (float)a;
    gscale[(size_t)k * C + c] = (float)b;
}

__global__ __launch_bounds__(BN_T) void cond_bn_bwd_apply_kernel(
    const float *__restrict__ x, const float *__restrict__ gy, const int *__restrict__ labels, int N,
    int C, int HW, int S, int K, const float *__restrict__ scale, const float *__restrict__ offset,
    const float *__restrict__ save, const double *__restrict__ ab, float *__restrict__ gx) {
    const int c = blockIdx.x, s = blockIdx.y;
    __shared__ float sh[2];
    if (threadIdx.x < SMMD_WAVE) {
        // fixed order: lane-strided over the samples, then the wave tree
        double s1 = 0.0, s2 = 0.0;
        for (int n = threadIdx.x; n < N; n += SMMD_WAVE) {
            const double g = (double)scale[(size_t)cbn_label(labels, n, K) * C + c];
            s1 += g * ab[((size_t)n * C + c) * 2 + 0];
            s2 += g * ab[((size_t)n * C + c) * 2 + 1];
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (threadIdx.x == 0) {
            const double cnt = (double)N * (double)HW;
            sh[0] = (float)(s1 / cnt);
            sh[1] = (float)(s2 / cnt);
        }
    }
    __syncthreads();
    const float m1 = sh[0], m2 = sh[1];
    const float k = save[3 * c + 0], ms = save[3 * c + 1], inv = save[3 * c + 2];
    int n0, n1;
    bn_rows(N, S, s, n0, n1);
    const CbnLane ln(HW);
    if (ln.r >= ln.rpi) return;
    for (int n = n0 + ln.r; n < n1; n += ln.rpi) {
        const size_t e = (size_t)cbn_label(labels, n, K) * C + c;
        const float gm = scale[e], sc = gm * inv, bb = offset[e];
        const size_t off = ((size_t)n * C + c) * HW;
        const float4 *xr = reinterpret_cast<const float4 *>(x + off);
        const float4 *gr = reinterpret_cast<const float4 *>(gy + off);
        float4 *out = reinterpret_cast<float4 *>(gx + off);
        for (int i = ln.col; i < ln.w4; i += ln.step) {
            const float4 v = xr[i], g = gr[i];
            float gz, xh;
            float4 o;
            cbn_bwd_elem(v.x, g.x, k, ms, inv, sc, bb, gz, xh); o.x = inv * ((gm * gz - m1) - xh * m2);
            cbn_bwd_elem(v.y, g.y, k, ms, inv, sc, bb, gz, xh); o.y = inv * ((gm * gz - m1) - xh * m2);
            cbn_bwd_elem(v.z, g.z, k, ms, inv, sc, bb, gz, xh); o.z = inv * ((gm * gz - m1) - xh * m2);
            cbn_bwd_elem(v.w, g.w, k, ms, inv, sc, bb, gz, xh); o.w = inv * ((gm * gz - m1) - xh * m2);
            out[i] = o;
        }
    }
}

inline size_t cbn_part_bytes(int N, int C) {
    return (size_t)bn_split(N, C) * C * 2 * sizeof(double);
}

}  // namespace smmd

using namespace smmd;

// the statistics slab [S][C][2], then ab [N][C][2] of the backward (doubles)
extern "C" size_t smmd_cond_bn_relu_workspace_bytes(int N, int C) {
    if (N <= 0 || C <= 0) return 0;
    return cbn_part_bytes(N, C) + (size_t)N * C * 2 * sizeof(double);
}

extern "C" smmd_status smmd_cond_bn_relu_fwd(const float *x, const int32_t *labels, int N, int C,
                                             int HW, int num_classes, const float *scale,
                                             const float *offset, float eps, float *y, float *save,
                                             void *ws, size_t ws_bytes, smmd_stream_t stream) {
    if (!x || !labels || !scale || !offset || !y || !ws) return SMMD_EINVAL;
    if (N < 1 || C < 1 || HW < 4 || (HW & 3) || num_classes <= 0) return SMMD_EINVAL;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 7)) return SMMD_EINVAL;
    const int S = bn_split(N, C);
    if (S > 65535 || ws_bytes < smmd_cond_bn_relu_workspace_bytes(N, C)) return SMMD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double *part = static_cast<double *>(ws);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(C, S), dim3(BN_T), 0, st, x, N, C, HW, S, part);
    smmd_status e = last_launch_status();
    if (e != SMMD_OK) return e;
    hipLaunchKernelGGL(cond_bn_apply_kernel, dim3(C, S), dim3(BN_T), 0, st, x, labels, N, C, HW, S,
                       num_classes, (const double *)part, scale, offset, eps, y, save);
    return last_launch_status();
}

extern "C" smmd_status smmd_cond_bn_relu_bwd(const float *x, const float *gy, const int32_t *labels,
                                             int N, int C, int HW, int num_classes,
                                             const float *scale, const float *offset,
                                             const float *save, float *gx, float *gscale,
                                             float *goffset, void *ws, size_t ws_bytes,
                                             smmd_stream_t stream) {
    if (!x || !gy || !labels || !scale || !offset || !save || !gx || !gscale || !goffset || !ws)
        return SMMD_EINVAL;
    if (N < 1 || C < 1 || HW < 4 || (HW & 3) || num_classes <= 0) return SMMD_EINVAL;
    if (((uintptr_t)x & 15) || ((uintptr_t)gy & 15) || ((uintptr_t)gx & 15) || ((uintptr_t)ws & 7))
        return SMMD_EINVAL;
    const int S = bn_split(N, C);
    const int ct = (C + BN_T - 1) / BN_T;
    if (S > 65535 || ct > 65535 || ws_bytes < smmd_cond_bn_relu_workspace_bytes(N, C))
        return SMMD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double *ab = reinterpret_cast<double *>(static_cast<char *>(ws) + cbn_part_bytes(N, C));
    hipLaunchKernelGGL(cond_bn_bwd_rows_kernel, dim3(C, S), dim3(BN_T), 0, st, x, gy, labels, N, C,
                       HW, S, num_classes, scale, offset, save, ab);
    smmd_status e = last_launch_status();
    if (e != SMMD_OK) return e;
    hipLaunchKernelGGL(cond_bn_table_kernel, dim3(num_classes, ct), dim3(BN_T), 0, st,
                       (const double *)ab, labels, N, C, num_classes, gscale, goffset);
    e = last_launch_status();
    if (e != SMMD_OK) return e;
    hipLaunchKernelGGL(cond_bn_bwd_apply_kernel, dim3(C, S), dim3(BN_T), 0, st, x, gy, labels, N, C,
                       HW, S, num_classes, scale, offset, save, (const double *)ab, gx);
    return last_launch_status();
}
