// smmd_wino_common.hpp -- what the four Winograd sources (smmd_wino.hip,
// smmd_wino_s2.hip, smmd_wino_wgrad.hip, smmd_wino_s2_wgrad.hip) share: the
// vector types, the DPP neighbour moves, the 2 GiB buffer descriptor and the
// ordered slab reductions of their split launches.
//
// The reduction kernels take an empty tag type, one per entry point
// (anonymous-namespace structs of the including file), that nothing but the
// kernel's name depends on: a profile then says whose reduction ran
// (tools/pmc_traffic.py GROUPS), and each object holds its own instances.
#pragma once

#include "smmd_common.hpp"

namespace smmd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

// neighbour lanes' values, 0 where the source lane is outside the wave
// (bound_ctrl: no preset of the destination; every VALU instruction costs
// SIMD time beside the f32 MFMA, profiles/r12/mfma_valu_coissue.txt)
__device__ __forceinline__ float dpp_from_left(float v) {    // lane l gets lane l-1's v
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138,
                                                              0xf, 0xf, true));
}

__device__ __forceinline__ float dpp_from_right(float v) {   // lane l gets lane l+1's v
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130,
                                                              0xf, 0xf, true));
}

// buffer access: a wave-uniform base in the descriptor, the lane's 32-bit
// byte offset in one VGPR (no 64-bit address arithmetic per access).  The
// range is 0x7fffffff bytes and BUF_OOB = 2^31 its out-of-range sentinel: an
// offset at or past the range reads zeros and stores nothing.  Every tensor
// addressed this way is under 2 GiB: the `< 2^29` floats bounds of the
// *_supported functions.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc_2g(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7fffffff, 0x00020000);
}
constexpr uint32_t BUF_OOB = 0x80000000u;

// ---- ordered slab reductions ------------------------------------------------
// A split launch writes S partial results ("slabs") of n4 float4 each, one
// after the other; they are added in ascending slab order, starting from slab
// 0's value, so the result does not depend on how the slices were scheduled.

// out[i] = sum of the S slabs, in slab order
// (acc: out + the sum, a later gradient contribution added last: the same add
// autograd would run, convops._late_gw)
template <class Tag>
__global__ void slab_sum_kernel(const float4 *__restrict__ part, int S, int64_t n4,
                                float4 *__restrict__ out, int acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 a = part[i];
    for (int s = 1; s < S; ++s) {
        const float4 v = part[(int64_t)s * n4 + i];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    if (acc) {
        const float4 o = out[i];
        a = make_float4(o.x + a.x, o.y + a.y, o.z + a.z, o.w + a.w);
    }
    out[i] = a;
}

// the first level for many slabs: out[g] = slabs g G .. g G + G - 1, in order,
// one thread per (group, float4): the many-slice layers (the 64-channel 3x3
// weight gradient has 512) read their partials at the full width of the chip
template <class Tag>
__global__ void slab_group_kernel(const float4 *__restrict__ part, int S, int G, int64_t n4,
                                  int ngroups, float4 *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4 * ngroups) return;
    const int gi = (int)(idx / n4);
    const int64_t f = idx - (int64_t)gi * n4;
    const int s0 = gi * G, s1 = min(S, s0 + G);
    float4 a = part[(int64_t)s0 * n4 + f];
    for (int s = s0 + 1; s < s1; ++s) {
        const float4 v = part[(int64_t)s * n4 + f];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    out[idx] = a;
}

// a split convolution's output [N][K][HW] (HW % 4 == 0): the slabs in order,
// + bias[k], then relu (fmaxf) or the mask's select (mask <= 0 ? 0 : .,
// threshold_backward), then acc (y + the result).  The flags are wave-uniform.
template <class Tag>
__global__ void slab_reduce_bias_kernel(const float *__restrict__ part,
                                        const float *__restrict__ bias, float *__restrict__ y,
                                        int64_t n4, int S, int K, int HW, int relu,
                                        const float *__restrict__ mask, int acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 *p4 = reinterpret_cast<const float4 *>(part);
    const float4 mv = mask ? reinterpret_cast<const float4 *>(mask)[i] : float4{};
    float4 s = p4[i];
    for (int z = 1; z < S; ++z) {
        const float4 t = p4[i + z * n4];
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    if (bias) {
        const float b = bias[(int)((i * 4 / HW) % K)];
        s.x += b; s.y += b; s.z += b; s.w += b;
    }
    if (relu) {
        s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f);
    } else if (mask) {
        s.x = mv.x <= 0.f ? 0.f : s.x;
        s.y = mv.y <= 0.f ? 0.f : s.y;
        s.z = mv.z <= 0.f ? 0.f : s.z;
        s.w = mv.w <= 0.f ? 0.f : s.w;
    }
    if (acc) {
        const float4 o = reinterpret_cast<const float4 *>(y)[i];
        s = make_float4(o.x + s.x, o.y + s.y, o.z + s.z, o.w + s.w);
    }
    reinterpret_cast<float4 *>(y)[i] = s;
}

template <class Tag>
inline smmd_status slab_reduce_bias(const float *part, const float *bias, float *y, int64_t n4,
                                    int S, int K, int HW, int relu, const float *mask, int acc,
                                    hipStream_t st) {
    slab_reduce_bias_kernel<Tag><<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st>>>(
        part, bias, y, n4, S, K, HW, relu, mask, acc);
    return last_launch_status();
}

// slices of a weight gradient's tile reduction for `blocks` (k, c) blocks:
// 256 workgroups in all, at least min_chunks chunks per slice
inline int slab_slices(int blocks, int64_t nchunks, int min_chunks) {
    int64_t S = (256 + blocks - 1) / blocks;
    S = min(S, max((int64_t)1, nchunks / min_chunks));
    return (int)max((int64_t)1, S);
}

constexpr int SLAB_GROUP = 16;                     // slabs per first-level group

// groups of the first level (0: one level); a workspace of S slabs holds
// S + slab_groups(S)
inline int slab_groups(int S) { return S > 2 * SLAB_GROUP ? (S + SLAB_GROUP - 1) / SLAB_GROUP : 0; }

// The group level, where Sused slabs are enough for one: the groups' sums go
// to the scratch after the Salloc slabs the workspace was sized for, and
// part / Sused become what is left for the last level to add.
template <class Tag>
inline smmd_status slab_group_level(float *&part, int &Sused, int Salloc, int64_t n4,
                                    hipStream_t st) {
    const int ng = slab_groups(Sused);
    if (ng == 0) return SMMD_OK;
    float *grp = part + (size_t)Salloc * n4 * 4;
    const int64_t nt = n4 * ng;
    slab_group_kernel<Tag><<<dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st>>>(
        reinterpret_cast<const float4 *>(part), Sused, SLAB_GROUP, n4, ng,
        reinterpret_cast<float4 *>(grp));
    part = grp;
    Sused = ng;
    return last_launch_status();
}

// out (+)= the Sused slabs at part, in order: the group level if there are
// many, then the sum
template <class Tag>
inline smmd_status slab_sum(float *part, int Sused, int Salloc, int64_t n4, float *out, int acc,
                            hipStream_t st) {
    const smmd_status e = slab_group_level<Tag>(part, Sused, Salloc, n4, st);
    if (e != SMMD_OK) return e;
    slab_sum_kernel<Tag><<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st>>>(
        reinterpret_cast<const float4 *>(part), Sused, n4, reinterpret_cast<float4 *>(out), acc);
    return last_launch_status();
}

}  // namespace smmd
