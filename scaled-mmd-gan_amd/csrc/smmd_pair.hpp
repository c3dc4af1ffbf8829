// smmd_pair.hpp -- the per-pair kernel evaluator of the lane-owns-a-row sweeps
// (smmd_mmd_tile.hip, smmd_ratio.hip): the Gaussian and rational-quadratic
// families in their fast forms (term count a template constant), the other
// kinds through the shared evaluator of smmd_kern.hpp.
#pragma once
#include "smmd_common.hpp"
#include "smmd_kern.hpp"

namespace smmd {

template <int DT>
__device__ __forceinline__ float tdot(const float (&a)[DT], const float (&b)[DT]) {
    float s = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < DT; ++k) s = fmaf(a[k], b[k], s);
    return s;
}

// Per pair: K, and (al, be) with dK/dz_i = al z_i + be (z_i - z_j).
// NT > 0: Gaussian / RQ mixture of NT terms in the fast form; NT == 0: the
// shared evaluator of smmd_kern.hpp (runtime term count; distance, dot).
template <int KIND, int NT>
struct PairEval {
    float p0[NT > 0 ? NT : 1], p1[NT > 0 ? NT : 1], p2[NT > 0 ? NT : 1];
    float add_dot;
    __device__ __forceinline__ void init(const KParams &kp) {
        add_dot = kp.add_dot;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (KIND == SMMD_KIND_RBF) {
                p0[t] = kp.c1[t] * 1.4426950408889634f;   // -gamma log2(e)
                p1[t] = kp.wt[t];
                p2[t] = 2.f * kp.c1[t];                   // d/draw, x2 (d raw / d z)
            } else {
                p0[t] = 1.f / kp.c1[t];                   // 1 / (2 alpha)
                p1[t] = kp.c2[t];                         // -alpha
                p2[t] = kp.wt[t];
            }
        }
    }
    __device__ __forceinline__ void eval(const KParams &kp, float raw, float dot, float sqi,
                                         float sqc, float &K, float &al, float &be) const {
        if (NT == 0) {
            Kern<KIND>::eval(kp, raw, dot, sqi, sqc, K, al, be);
        } else if (KIND == SMMD_KIND_RBF) {     // mmd.py:55-116
            const float R = fmaxf(raw, 0.f);
            float k = 0.f, dk = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float e = p1[t] * __builtin_amdgcn_exp2f(p0[t] * R);
                k += e;
                dk = fmaf(p2[t], e, dk);
            }
            K = k;
            al = 0.f;
            be = (raw >= 0.f) ? dk : 0.f;         // tf.maximum: ties pass the gradient
        } else {                                  // RQ, mmd.py:143-188
            const float R = fmaxf(raw, 0.f);
            float k = 0.f, dk = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float q = fmaf(R, p0[t], 1.f);
                const float e = p2[t] * __builtin_amdgcn_exp2f(p1[t] * __builtin_amdgcn_logf(q));
                k += e;
                // d e / dR = e * (-alpha) / (q * 2 alpha)
                dk = fmaf(e * (p1[t] * p0[t]), __builtin_amdgcn_rcpf(q), dk);
            }
            if (add_dot > 0.f) k = fmaf(add_dot, dot, k);
            K = k;
            al = add_dot;
            be = ((raw >= 0.f) ? 2.f * dk : 0.f) - add_dot;
        }
    }
};

}  // namespace smmd
