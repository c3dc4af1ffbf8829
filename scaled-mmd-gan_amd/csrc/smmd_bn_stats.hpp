// smmd_bn_stats.hpp -- the batch statistics pass shared by the batch norm +
// ReLU kernels (smmd_bnrelu.hip) and their class-conditional form
// (smmd_cond_bn.hip): the (C, S) grid's row split and the shifted channel sums.
#pragma once

#include "smmd_common.hpp"

namespace smmd {

constexpr int BN_T = 256;

__device__ __forceinline__ void bn_rows(int N, int S, int s, int &n0, int &n1) {
    const int R = (N + S - 1) / S;
    n0 = s * R;
    n1 = min(N, n0 + R);
}

static __global__ __launch_bounds__(BN_T) void bn_stats_kernel(const float *__restrict__ x, int N,
                                                               int C, int HW, int S,
                                                               double *__restrict__ part) {
    const int c = blockIdx.x, s = blockIdx.y;
    int n0, n1;
    bn_rows(N, S, s, n0, n1);
    const int w4 = HW >> 2;
    // rows shorter than the block are packed rpi per step (lane t: row t / w4,
    // column t % w4), so every lane loads on the small maps too
    const int rpi = w4 >= BN_T ? 1 : BN_T / w4;
    const int r = w4 >= BN_T ? 0 : (int)threadIdx.x / w4;
    const int col = w4 >= BN_T ? (int)threadIdx.x : (int)threadIdx.x - r * w4;
    const int step = w4 >= BN_T ? BN_T : w4;     // column stride within a row
    // shifted sums: every thread subtracts the channel's first element k
    // (x[0, c, 0], one cached load), so sum (x - k)^2 does not cancel
    // against the mean when |mean| >> std (a sample lies within a few std
    // of the mean); apply adds k back
    const float k = x[(size_t)c * HW];
    float a = 0.f, q = 0.f;
    if (r < rpi) {
        for (int n = n0 + r; n < n1; n += rpi) {
            const float4 *row = reinterpret_cast<const float4 *>(x + ((size_t)n * C + c) * HW);
            for (int i = col; i < w4; i += step) {
                const float4 v = row[i];
                const float dx = v.x - k, dy = v.y - k, dz = v.z - k, dw = v.w - k;
                a += (dx + dy) + (dz + dw);
                q = fmaf(dx, dx, q);
                q = fmaf(dy, dy, q);
                q = fmaf(dz, dz, q);
                q = fmaf(dw, dw, q);
            }
        }
    }
    __shared__ double red[BN_T / SMMD_WAVE];
    const double sa = block_sum<BN_T / SMMD_WAVE>((double)a, red);
    const double sq = block_sum<BN_T / SMMD_WAVE>((double)q, red);
    if (threadIdx.x == 0) {
        part[((size_t)s * C + c) * 2 + 0] = sa;
        part[((size_t)s * C + c) * 2 + 1] = sq;
    }
}

inline int bn_split(int N, int C) {
    if (C >= 512) return 1;
    int S = (2048 + C - 1) / C;
    if (S > N) S = N;
    return S < 1 ? 1 : S;
}

}  // namespace smmd
