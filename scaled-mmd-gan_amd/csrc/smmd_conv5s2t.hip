// smmd_conv5s2t.hip -- the wide 5x5 stride-2 transposed convolutions of the
// DCGAN generators (architecture.py's deconv2d stack, snops.Deconv2d(cin, cout,
// 5, 2): 1024@2 ... 128@16 -> 64@32) on the f32 MFMA, fp32 NCHW:
//
//   y[n, co, oh, ow] = bias[co] + sum_{ci, kh, kw} x[n, ci, ih, iw] w[ci, co, kh, kw]
//   over all (ih, kh) with oh = 2 ih + kh - 1, ow likewise; y is [n, cout, 2h, 2w]
//
// = conv_transpose2d(x, w, b, 2, 1)[:, :, :2h, :2w], the TF SAME geometry (one
// zero row before, two after).  w is read as Deconv2d stores it, [cin, cout, 5,
// 5]: no transformed copy, no filter launch.
//
// The layers have many channels and 2x2 .. 32x32 images, so the pixel dimension
// of the implicit GEMM is the flattened input grid (n, r, c), as in
// smmd_conv5s2.hip: the batch fills the tile where the image cannot.
//
// c5t_kernel: block = 64 output channels x 64 input-grid pixels = 64 x 256
// output pixels, all four output parity phases; 4 waves, wave (mh, jh) the
// 32 x 32 quadrant of every phase on v_mfma_f32_32x32x2_f32 (4 x 16 = 64
// accumulator registers).  Output pixel (2r + a, 2c + b) reads input rows
// r - 1 .. r + 1 only: tap kh of row parity a reads row r + dr with
// kh = a + 1 - 2 dr (a = 0: kh 3, 1; a = 1: kh 4, 2, 0), columns likewise.  The
// reduction runs over input channels in chunks of CC = 4.  Per chunk
//   B: the tile plus a one-pixel halo of each channel of x is staged in LDS
//      once, as rows of the image deduplicated over the tile's pixel rows
//      (staged row = n (h + 2) + row + 1, w + 2 floats), zeros outside the
//      image.  The channel stride is 32 mod 64 floats: the two lane halves (the
//      two channels of a pair) read disjoint banks.
//   A: the chunk's weights of the block's 64 output channels are one contiguous
//      run of 64 x 25 floats per input channel of w as stored: float4 loads,
//      float4 LDS stores, staged as they lie, channel stride 1600 + 32.  Lane
//      (h, l32) reads [channel 2q + h][row l32][tap]: row stride 25 (odd), the
//      halves 32 banks apart: conflict-free.
//   For a channel pair the wave reads the 9 shifted views (dr, dc) of its
//   pixel column once and issues every tap that maps to a view on it:
//   3.3 + 3.2 + 2.3 + 2.2 = 25 MFMAs on 9 B reads; no zero is multiplied.
//   MFMA t reduces over (channel 2q, tap t) in lane half 0 and (channel 2q + 1,
//   tap t) in half 1.
// Both stages are double-buffered: the next chunk's global loads are issued
// before the current chunk's MFMAs and stored to the other buffer after them.
// The source offsets of a thread's staged elements are formed once per block.
// Epilogue: a lane's accumulators of column parities b = 0, 1 are adjacent
// output columns: bias added, one float2 store per channel on each of the two
// output rows (32 lanes: 256 contiguous bytes).
// With few tiles (512@2x2 at batch 64 -> 256: 16 of them) the reduction is
// split over channel groups (blockIdx.y), a function of the shape only; the
// partial outputs go to the workspace and are added in slice order (slab_sum),
// the bias in slice 0.
//
// Accumulation order: fixed (chunks, pairs, views, taps, then slices in order),
// no float atomics: two runs give the same bits.
//
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950), c5t_kernel: 98 VGPRs +
// 64 AGPRs (the accumulators), 57 SGPRs, no scratch, no spills, occupancy 3
// waves / SIMD by registers.  LDS is dynamic, 2 x 4 x (1632 + channel stride)
// floats: 57,344 to 61,440 bytes on the generator shapes (2x2 .. 32x32: two
// blocks per CU), 69,632 at the widest image the stage takes.
#include "smmd_wino_common.hpp"

namespace smmd {

namespace {

struct C5TSum {};

constexpr int C5T_T = 256;
constexpr int C5T_CC = 4;                         // input channels per chunk
constexpr int C5T_EMAX = 2;                       // staged x floats / 256 per channel
constexpr int C5T_AQ = 64 * 25 / 4;               // float4 per input channel of the A run
constexpr int C5T_ACS = 64 * 25 + 32;             // A stage: floats per input channel
constexpr int C5T_NA = (C5T_CC * C5T_AQ + C5T_T - 1) / C5T_T;
constexpr int C5T_CUS = 256;

struct C5TArgs {
    int N, Cin, Cout, H, W;
    int pstride;                   // B stage: floats per input channel
    int cps;                       // chunks per reduction slice
    long long slab;                // floats per partial output
};

__global__ __launch_bounds__(C5T_T) void c5t_kernel(const float *__restrict__ wgt,
                                                    const float *__restrict__ x,
                                                    const float *__restrict__ bias,
                                                    float *__restrict__ y, C5TArgs p) {
    extern __shared__ __attribute__((aligned(16))) float c5t_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int rpi = p.H + 2, RS = p.W + 2;      // staged rows per image, staged row length
    const int J = p.N * p.H * p.W;
    const int mb_n = p.Cout / 64;
    const int mb = blockIdx.x % mb_n, jb = blockIdx.x / mb_n;
    const int m0 = mb * 64, j0 = jb * 64;
    const int STAGE = C5T_CC * (C5T_ACS + p.pstride);

    // the tile's staged rows: [S0, S0 + SR) of the (image, row) sequence
    const int jl = min(j0 + 63, J - 1);
    const int ga = j0 / p.W, gb = jl / p.W;
    const int S0 = (ga / p.H) * rpi + ga % p.H;
    const int SR = (gb / p.H) * rpi + gb % p.H + 3 - S0;
    const int npatch = SR * RS;
    if (npatch > p.pstride || npatch > C5T_EMAX * C5T_T) return;   // (the host's bound: never)

    const int plane = p.H * p.W;
    int goff[C5T_EMAX];            // staged element -> offset into channel 0 of x, -1: zero
#pragma unroll
    for (int k = 0; k < C5T_EMAX; ++k) {
        const int e = tid + C5T_T * k;
        goff[k] = -1;
        if (e < npatch) {
            const int s = S0 + e / RS, iw = e % RS - 1;
            const int n = s / rpi, ih = s - n * rpi - 1;
            if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
                goff[k] = n * p.Cin * plane + ih * p.W + iw;
        }
    }
    const int s = blockIdx.y;
    const int cbeg = s * p.cps;
    const int nchunk = min(p.cps, p.Cin / C5T_CC - cbeg);

    f4v ga4[C5T_NA];
    float gx[C5T_CC][C5T_EMAX];
    auto gload = [&](int c) {
        const int ch0 = (cbeg + min(c, nchunk - 1)) * C5T_CC;
#pragma unroll
        for (int i = 0; i < C5T_NA; ++i) {
            const int f = min(tid + C5T_T * i, C5T_CC * C5T_AQ - 1);
            const int ch = f / C5T_AQ, quad = f - ch * C5T_AQ;
            ga4[i] = *reinterpret_cast<const f4v *>(
                wgt + ((int64_t)(ch0 + ch) * p.Cout + m0) * 25 + 4 * quad);
        }
        const float *xc = x + (int64_t)ch0 * plane;
#pragma unroll
        for (int ch = 0; ch < C5T_CC; ++ch)
#pragma unroll
            for (int k = 0; k < C5T_EMAX; ++k)
                gx[ch][k] = goff[k] >= 0 ? xc[(int64_t)ch * plane + goff[k]] : 0.f;
    };
    auto lstore = [&](int buf) {
        float *As_ = c5t_lds + buf * STAGE;
        float *Bs_ = As_ + C5T_CC * C5T_ACS;
#pragma unroll
        for (int i = 0; i < C5T_NA; ++i) {
            const int f = tid + C5T_T * i;
            const int ch = f / C5T_AQ, quad = f - ch * C5T_AQ;
            if (f < C5T_CC * C5T_AQ)
                *reinterpret_cast<f4v *>(As_ + ch * C5T_ACS + 4 * quad) = ga4[i];
        }
#pragma unroll
        for (int ch = 0; ch < C5T_CC; ++ch)
#pragma unroll
            for (int k = 0; k < C5T_EMAX; ++k) {
                const int e = tid + C5T_T * k;
                if (e < npatch) Bs_[ch * p.pstride + e] = gx[ch][k];
            }
    };

    const int mh = wv >> 1, jh = wv & 1, h = lane >> 5, l32 = lane & 31;
    // this lane's pixel column (a column past the end reads the last one's
    // operands and stores nothing)
    const int j = j0 + jh * 32 + l32;
    const int jc = min(j, J - 1);
    const int gr = jc / p.W, pc = jc - gr * p.W;
    const int pn = gr / p.H, pr = gr - pn * p.H;
    // view (dr, dc) of the pixel is at + (dr + 1) RS + (dc + 1)
    const int boff = (pn * rpi + pr - S0) * RS + pc + h * p.pstride;
    const int aoff = h * C5T_ACS + (mh * 32 + l32) * 25;
    f32x16 acc[2][2] = {{f32x16{}, f32x16{}}, {f32x16{}, f32x16{}}};   // [a][b]

    gload(0);
    lstore(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        gload(c + 1);
        const float *As_ = c5t_lds + (c & 1) * STAGE;
        const float *Bs_ = As_ + C5T_CC * C5T_ACS;
#pragma unroll
        for (int q = 0; q < C5T_CC / 2; ++q) {
            const float *ap = As_ + aoff + 2 * q * C5T_ACS;
            const float *bp = Bs_ + boff + 2 * q * p.pstride;
#pragma unroll
            for (int i = 0; i < 3; ++i) {           // dr = i - 1
                const float *br = bp + i * RS;
#pragma unroll
                for (int l = 0; l < 3; ++l) {       // dc = l - 1
                    const float bv = br[l];
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const int kh = a + 3 - 2 * i;
                        if (kh < 0 || kh > 4) continue;
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const int kw = b + 3 - 2 * l;
                            if (kw < 0 || kw > 4) continue;
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kh * 5 + kw], bv,
                                                                             acc[a][b], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (c + 1 < nchunk) {
            lstore((c + 1) & 1);
            __syncthreads();
        }
    }

    // epilogue: lane (h, l32) holds rows (r & 3) + 8 (r >> 2) + 4 h of the four
    // phases of pixel column j: output rows 2 pr, 2 pr + 1, columns 2 pc, 2 pc + 1
    if (j >= J) return;
    const int Wo = 2 * p.W;
    const int64_t oplane = 4 * (int64_t)plane;
    float *yc = y + (int64_t)s * p.slab + (int64_t)pn * p.Cout * oplane + (2 * pr) * Wo + 2 * pc;
    const int mr = m0 + mh * 32 + 4 * h;
    const bool hb = bias != nullptr && s == 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mr + (r & 3) + 8 * (r >> 2);
        const float bv = hb ? bias[m] : 0.f;
        float *d = yc + (int64_t)m * oplane;
        *reinterpret_cast<float2 *>(d) = make_float2(acc[0][0][r] + bv, acc[0][1][r] + bv);
        *reinterpret_cast<float2 *>(d + Wo) = make_float2(acc[1][0][r] + bv, acc[1][1][r] + bv);
    }
}

bool c5t_aligned(const void *q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

// most staged floats per channel of a run of 64 pixels of an h x w grid: the
// pixel rows it touches, one halo row on each side, two more per image
// boundary crossed, w + 2 floats each
int c5t_patch(int h, int w) {
    const int gr = (63 + w - 1) / w + 1;
    const int bnd = (gr - 1 + h - 1) / h;
    return (gr + 2 + 2 * bnd) * (w + 2);
}

// the B stage's channel stride: >= the patch, 32 mod 64
int c5t_pstride(int h, int w) { return (c5t_patch(h, w) + 31) / 64 * 64 + 32; }

bool c5t_ok(int n, int cin, int cout, int h, int w) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return false;
    if (cin % C5T_CC || cout % 64 || w > 4096) return false;
    const int64_t lim = 1ll << 29;
    if ((int64_t)n * cin * h * w >= lim || (int64_t)n * cout * h * w * 4 >= lim ||
        (int64_t)cin * cout * 25 >= lim)
        return false;
    return c5t_patch(h, w) <= C5T_EMAX * C5T_T;
}

int c5t_slices(int n, int cin, int cout, int h, int w) {
    const int64_t tiles = ((int64_t)n * h * w + 63) / 64 * (cout / 64);
    return tiles >= C5T_CUS ? 1 : slab_slices((int)tiles, cin / C5T_CC, 4);
}

}  // namespace

}  // namespace smmd

using namespace smmd;

extern "C" int smmd_conv5s2t_supported(int n, int cin, int cout, int h, int w) {
    return c5t_ok(n, cin, cout, h, w);
}

extern "C" size_t smmd_conv5s2t_workspace_bytes(int n, int cin, int cout, int h, int w) {
    if (!c5t_ok(n, cin, cout, h, w)) return 0;
    const int S = c5t_slices(n, cin, cout, h, w);
    return S > 1 ? (size_t)(S + slab_groups(S)) * n * cout * h * w * 4 * sizeof(float) : 0;
}

extern "C" smmd_status smmd_conv5s2t(const float *x, const float *wgt, const float *bias, float *y,
                                     int n, int cin, int cout, int h, int w, void *ws,
                                     size_t ws_bytes, smmd_stream_t stream) {
    if (!x || !wgt || !y) return SMMD_EINVAL;
    if (!c5t_ok(n, cin, cout, h, w)) return SMMD_EUNSUPPORTED;
    if (!c5t_aligned(wgt, 16) || !c5t_aligned(y, 16)) return SMMD_EINVAL;
    const int S = c5t_slices(n, cin, cout, h, w);
    const size_t need = smmd_conv5s2t_workspace_bytes(n, cin, cout, h, w);
    if (need && (!ws || ws_bytes < need || !c5t_aligned(ws, 16))) return SMMD_EINVAL;
    const int nch = cin / C5T_CC;
    C5TArgs p{};
    p.N = n; p.Cin = cin; p.Cout = cout; p.H = h; p.W = w;
    p.pstride = c5t_pstride(h, w);
    p.cps = (nch + S - 1) / S;
    const int nslices = (nch + p.cps - 1) / p.cps;
    p.slab = (long long)n * cout * h * w * 4;
    const size_t lds = 2 * (size_t)C5T_CC * (C5T_ACS + p.pstride) * sizeof(float);
    static bool attr = false;                   // the stage may pass the default 64 KiB
    if (!attr) {
        const smmd_status e = hip_status(hipFuncSetAttribute(
            reinterpret_cast<const void *>(c5t_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
            (int)(2 * C5T_CC * (C5T_ACS + C5T_EMAX * C5T_T + 64) * sizeof(float))));
        if (e != SMMD_OK) return e;
        attr = true;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t tiles = ((int64_t)n * h * w + 63) / 64;
    float *part = nslices > 1 ? static_cast<float *>(ws) : y;
    c5t_kernel<<<dim3((unsigned)(tiles * (cout / 64)), (unsigned)nslices), dim3(C5T_T), lds, st>>>(
        wgt, x, bias, part, p);
    const smmd_status e = last_launch_status();
    if (e != SMMD_OK || nslices == 1) return e;
    return slab_sum<C5TSum>(part, nslices, S, p.slab / 4, y, 0, st);
}
