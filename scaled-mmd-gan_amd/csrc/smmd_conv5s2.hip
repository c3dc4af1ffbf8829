// smmd_conv5s2.hip -- the 5x5 stride-2 convolutions of the DCGAN critics
// (architecture.py:323-343, snops.conv2d) on the f32 MFMA, fp32 NCHW: forward,
// input gradient and weight gradient.  The layers have many channels and very
// small images (512 -> 1024 at 4 x 4 -> 2 x 2), so all three are direct
// implicit GEMMs whose pixel dimension is the flattened (n, row, column): the
// batch fills the tile where the image cannot.
//
// c5_gemm (forward and input gradient): block = 64 output channels x 64
// pixels, 4 waves, wave (mh, jh) the 32 x 32 quadrant on v_mfma_f32_32x32x2_f32.
// The reduction runs over (channel, tap) in chunks of CC channels.  Per chunk
//   B: the tile's receptive field of each channel is staged in LDS once, as
//      rows of the source image deduplicated over the tile's output rows
//      (staged row = n * rpi + rstep * row + tap row), zero where the tap is
//      outside the image.  Forward: a staged row holds the even input columns,
//      then the odd ones, so the stride-2 reads of the 5 taps of a row are
//      unit-stride over the lanes within a plane; the 25 taps are served from
//      that one stage.  Input gradient: one output parity phase per block
//      (blockIdx.z; 3x3, 3x2, 2x3, 2x2 taps, no zero is multiplied), the
//      pixels are (n, ih / 2, iw / 2) of the phase and the gy rows are
//      unit-stride as they are.
//   A: the chunk's weights, rows contiguous in global memory (forward: w as
//      stored, [cout][cin 25]; input gradient: the phase-sorted transpose
//      [cin][cout taps] written by c5_filter_kernel), float4 loads, staged
//      [row][CC taps] with an odd row stride (conflict-free column reads).
//   MFMA t of a channel pair reduces over (channel 2q, tap t) in lane half 0
//   and (channel 2q + 1, tap t) in half 1.
// Both stages are double-buffered: the next chunk's global loads are issued
// before the current chunk's MFMAs and stored to the other buffer after them.
// The source offsets of a thread's staged elements are formed once per block
// (they do not depend on the chunk).  With few tiles the reduction is split
// over channel groups (blockIdx.y); the partial outputs are added in slice
// order (slab_sum).
//
// c5_wgrad: block = 64 output channels x (8 input channels x 25 taps = 200
// columns, 7 groups of 32), the reduction over pixels in chunks of whole
// output rows (~64 pixels); wave (mh, ch) holds the 32-channel half mh of
// column groups ch, ch + 2, ch + 4 (, 6).  A = gy [co][pixel], B = the same
// parity-split x patch as the forward: a lane's column (ci, kh, kw) is a fixed
// offset into the patch and the pixel walks along staged rows.  The pixel
// range is split over blocks by row slices, summed in slice order.
//
// Tile choice: 64 x 64 with one wave per quadrant (16 accumulator registers)
// rather than 128 x 64: the deep layers have 128-256 pixels at batch 64, and
// the smaller tile gives twice the blocks before the reduction has to be
// split.  Resource use (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)
// and timings: see DESIGN.md section 5.
//
// Accumulation order: fixed (chunks in order, taps in order, slices in order),
// no float atomics: deterministic.
#include "smmd_wino_common.hpp"

namespace smmd {

namespace {

struct C5FwdSum {};
struct C5DxSum {};
struct C5WgSum {};

constexpr int C5_T = 256;
constexpr int C5_CC_FWD = 4, C5_EMAX_FWD = 8;     // channels per chunk, staged floats / 256 per channel
constexpr int C5_CC_DX = 8, C5_EMAX_DX = 4;
constexpr int C5_WG_CI = 8, C5_WG_COLS = 25 * C5_WG_CI, C5_EMAX_WG = 8;
constexpr int C5_WG_NA = 32;                      // gy loads per thread and chunk
constexpr int C5_AS_FWD = 25 * C5_CC_FWD + 1;     // A stage row strides (odd)
constexpr int C5_AS_DX = 9 * C5_CC_DX + 1;

struct C5Args {
    int N, R, M;                   // batch, reduction channels, output-row channels
    int H, W, Ho, Wo, pt, pl;      // the convolution: input H x W, output Ho x Wo
    int patch;                     // LDS floats per staged channel
    int cps;                       // chunks per reduction slice
    int nslices;
    long long slab;                // floats per partial output
};

// the tile geometry of one direction (forward, or one phase of the input
// gradient): output pixels (n, r, c) of an Hp x Wp grid per image
struct C5Geo {
    int Hp, Wp;                    // pixel grid per image
    int rpi, rstep, krows;         // staged rows per image, per pixel row, per tap column
    int RS, PL;                    // staged row length, offset of the odd plane
    int r0, c0;                    // input gradient: first (ih + pt) / 2, (iw + pl) / 2 of the phase
};

template <int MODE>
__device__ __forceinline__ C5Geo c5_geo(const C5Args &p, int a, int b) {
    C5Geo g;
    if (MODE == 0) {
        g.Hp = p.Ho; g.Wp = p.Wo;
        g.rpi = 2 * p.Ho + 3; g.rstep = 2; g.krows = 5;
        g.RS = 2 * p.Wo + 3; g.PL = p.Wo + 2;
        g.r0 = g.c0 = 0;
    } else {
        g.r0 = (p.pt - a + 1) >> 1;
        g.c0 = (p.pl - b + 1) >> 1;
        g.Hp = (p.H - (2 * g.r0 + a - p.pt) + 1) >> 1;
        g.Wp = (p.W - (2 * g.c0 + b - p.pl) + 1) >> 1;
        g.rpi = g.Hp + 2; g.rstep = 1; g.krows = 3;
        g.RS = g.Wp + 2; g.PL = 0;
    }
    return g;
}

// element offset into channel 0 of image n of the source tensor for staged
// (image row r, position q), or -1 where the tap lies outside it
template <int MODE>
__device__ __forceinline__ int c5_src(const C5Args &p, const C5Geo &g, int n, int r, int q) {
    if (MODE == 0) {
        const int ih = r - p.pt;
        const int c = q < g.PL ? 2 * q : 2 * (q - g.PL) + 1;
        const int iw = c - p.pl;
        if (ih < 0 || ih >= p.H || iw < 0 || iw >= p.W) return -1;
        return n * p.R * p.H * p.W + ih * p.W + iw;
    }
    const int oh = g.r0 + r - 2, ow = g.c0 + q - 2;
    if (oh < 0 || oh >= p.Ho || ow < 0 || ow >= p.Wo) return -1;
    return n * p.R * p.Ho * p.Wo + oh * p.Wo + ow;
}

template <int MODE, int CC, int EMAX, int TH, int TW>
__device__ __forceinline__ void c5_tile(const float *__restrict__ A, const float *__restrict__ X,
                                        const float *__restrict__ bias, float *__restrict__ Y,
                                        const C5Args &p, int a, int b, float *lds) {
    constexpr int T = TH * TW;                  // taps
    constexpr int ARL = CC * T;                 // A floats per row and chunk
    constexpr int AQ = ARL / 4;                 // float4 per row
    constexpr int AS = (MODE == 0 ? C5_AS_FWD : C5_AS_DX);
    constexpr int NA = (64 * AQ + C5_T - 1) / C5_T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const C5Geo g = c5_geo<MODE>(p, a, b);
    const int J = p.N * g.Hp * g.Wp;
    const int mb_n = p.M / 64;
    const int mb = blockIdx.x % mb_n, jb = blockIdx.x / mb_n;
    const int m0 = mb * 64, j0 = jb * 64;
    if (j0 >= J) return;                        // a phase with fewer tiles
    const int STAGE = 64 * AS + CC * p.patch;

    // the tile's staged rows: [S0, S0 + SR) of the (image, row) sequence
    const int jl = min(j0 + 63, J - 1);
    const int ga = j0 / g.Wp, gb = jl / g.Wp;
    const int S0 = (ga / g.Hp) * g.rpi + g.rstep * (ga % g.Hp);
    const int SR = (gb / g.Hp) * g.rpi + g.rstep * (gb % g.Hp) + g.krows - S0;
    const int npatch = SR * g.RS;
    if (npatch > p.patch || npatch > EMAX * C5_T) return;   // (the host's bound: never)

    const int plane = MODE == 0 ? p.H * p.W : p.Ho * p.Wo;
    int goff[EMAX];
#pragma unroll
    for (int k = 0; k < EMAX; ++k) {
        const int e = tid + C5_T * k;
        goff[k] = -1;
        if (e < npatch) {
            const int s = S0 + e / g.RS, q = e % g.RS;
            goff[k] = c5_src<MODE>(p, g, s / g.rpi, s % g.rpi, q);
        }
    }
    // A: row f / AQ, quad f % AQ of the chunk's 64 x ARL block
    const int64_t arow_g = (int64_t)p.R * T;
    const float *Ap = A;
    if (MODE == 1) {
        const int poff = a == 0 ? (b == 0 ? 0 : 9) : (b == 0 ? 15 : 21);
        Ap += (int64_t)poff * p.R * p.M;
    }
    const int s = blockIdx.y;
    const int cbeg = s * p.cps;
    const int nchunk = min(p.cps, p.R / CC - cbeg);

    float4 ga4[NA];
    float gx[CC][EMAX];
    auto gload = [&](int c) {
        const int ch0 = (cbeg + min(c, nchunk - 1)) * CC;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int f = min(tid + C5_T * i, 64 * AQ - 1);
            ga4[i] = *reinterpret_cast<const float4 *>(Ap + (int64_t)(m0 + f / AQ) * arow_g +
                                                       (int64_t)ch0 * T + 4 * (f % AQ));
        }
        const float *xc = X + (int64_t)ch0 * plane;
#pragma unroll
        for (int ch = 0; ch < CC; ++ch)
#pragma unroll
            for (int k = 0; k < EMAX; ++k)
                gx[ch][k] = goff[k] >= 0 ? xc[(int64_t)ch * plane + goff[k]] : 0.f;
    };
    auto lstore = [&](int buf) {
        float *As_ = lds + buf * STAGE;
        float *Bs_ = As_ + 64 * AS;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int f = tid + C5_T * i;
            if (f < 64 * AQ) {
                float *d = As_ + (f / AQ) * AS + 4 * (f % AQ);
                d[0] = ga4[i].x; d[1] = ga4[i].y; d[2] = ga4[i].z; d[3] = ga4[i].w;
            }
        }
#pragma unroll
        for (int ch = 0; ch < CC; ++ch)
#pragma unroll
            for (int k = 0; k < EMAX; ++k) {
                const int e = tid + C5_T * k;
                if (e < npatch) Bs_[ch * p.patch + e] = gx[ch][k];
            }
    };

    const int mh = w >> 1, jh = w & 1, h = lane >> 5, l32 = lane & 31;
    // this lane's pixel column (a column past the end reads the last one's
    // operands and stores nothing)
    const int j = j0 + jh * 32 + l32;
    const int jc = min(j, J - 1);
    const int gr = jc / g.Wp, pc = jc - gr * g.Wp;
    const int pn = gr / g.Hp, pr = gr - pn * g.Hp;
    const int bpix = (pn * g.rpi + g.rstep * pr - S0) * g.RS + pc + h * p.patch;
    const int aoff = (mh * 32 + l32) * AS + h * T;
    f32x16 acc = f32x16{};

    gload(0);
    lstore(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        gload(c + 1);
        const float *As_ = lds + (c & 1) * STAGE;
        const float *Bs_ = As_ + 64 * AS;
#pragma unroll
        for (int q = 0; q < CC / 2; ++q) {
            const float *ap = As_ + aoff + 2 * q * T;
            const float *bp = Bs_ + bpix + 2 * q * p.patch;
#pragma unroll
            for (int i = 0; i < TH; ++i) {
                const float *br = bp + (MODE == 0 ? i : 2 - i) * g.RS;
#pragma unroll
                for (int l = 0; l < TW; ++l) {
                    const float bv = MODE == 0 ? br[(l & 1) * g.PL + (l >> 1)] : br[2 - l];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[i * TW + l], bv, acc, 0, 0, 0);
                }
            }
        }
        if (c + 1 < nchunk) {
            lstore((c + 1) & 1);
            __syncthreads();
        }
    }

    // epilogue: lane (h, l32) holds rows (r & 3) + 8 (r >> 2) + 4 h of column j
    if (j >= J) return;
    float *yc = Y + (int64_t)s * p.slab;
    int64_t rstride;
    if (MODE == 0) {
        rstride = (int64_t)p.Ho * p.Wo;
        yc += (int64_t)pn * p.M * rstride + pr * p.Wo + pc;
    } else {
        rstride = (int64_t)p.H * p.W;
        yc += (int64_t)pn * p.M * rstride + (2 * (g.r0 + pr) + a - p.pt) * p.W +
              (2 * (g.c0 + pc) + b - p.pl);
    }
    const int mr = m0 + mh * 32 + 4 * h;
    const bool hb = MODE == 0 && bias != nullptr && s == 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mr + (r & 3) + 8 * (r >> 2);
        yc[(int64_t)m * rstride] = acc[r] + (hb ? bias[m] : 0.f);
    }
}

__global__ __launch_bounds__(C5_T) void c5_fwd_kernel(const float *__restrict__ wgt,
                                                      const float *__restrict__ x,
                                                      const float *__restrict__ bias,
                                                      float *__restrict__ y, C5Args p) {
    extern __shared__ float c5_lds[];
    c5_tile<0, C5_CC_FWD, C5_EMAX_FWD, 5, 5>(wgt, x, bias, y, p, 0, 0, c5_lds);
}

// blockIdx.z: the phase (a, b) = ((ih + pt) & 1, (iw + pl) & 1) of the input pixels
__global__ __launch_bounds__(C5_T) void c5_dx_kernel(const float *__restrict__ wt,
                                                     const float *__restrict__ gy,
                                                     float *__restrict__ gx, C5Args p) {
    extern __shared__ float c5_lds[];
    switch (blockIdx.z) {
    case 0: c5_tile<1, C5_CC_DX, C5_EMAX_DX, 3, 3>(wt, gy, nullptr, gx, p, 0, 0, c5_lds); break;
    case 1: c5_tile<1, C5_CC_DX, C5_EMAX_DX, 3, 2>(wt, gy, nullptr, gx, p, 0, 1, c5_lds); break;
    case 2: c5_tile<1, C5_CC_DX, C5_EMAX_DX, 2, 3>(wt, gy, nullptr, gx, p, 1, 0, c5_lds); break;
    default: c5_tile<1, C5_CC_DX, C5_EMAX_DX, 2, 2>(wt, gy, nullptr, gx, p, 1, 1, c5_lds); break;
    }
}

// the input gradient's A operand: wt[phase][ci][co][i][l] = w[co][ci][a + 2 i][b + 2 l],
// phases (a, b) in the order (0,0) (0,1) (1,0) (1,1) at 0, 9, 15, 21 x cin cout floats
__global__ void c5_filter_kernel(const float *__restrict__ w, float *__restrict__ wt, int cout,
                                 int cin) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)cout * cin * 25) return;
    const int tap = (int)(idx % 25);
    const int64_t cc = idx / 25;
    const int ci = (int)(cc % cin), co = (int)(cc / cin);
    const int kh = tap / 5, kw = tap - 5 * kh;
    const int a = kh & 1, i = kh >> 1, b = kw & 1, l = kw >> 1;
    const int TW = 3 - b, T = (3 - a) * TW;
    const int poff = a == 0 ? (b == 0 ? 0 : 9) : (b == 0 ? 15 : 21);
    wt[(int64_t)poff * cin * cout + ((int64_t)ci * cout + co) * T + i * TW + l] = w[idx];
}

struct C5WgArgs {
    int N, Ci, Co;
    int H, W, Ho, Wo, pt, pl;
    int patch;                     // LDS floats per staged channel
    int grc, cp, ast;              // output rows and (padded) pixels per chunk, A row stride
    int cps, accum;                // chunks per slice; one slice: add into gw
};

// partial gw of row slice blockIdx.y for 64 output channels x 8 input channels
__global__ __launch_bounds__(C5_T) void c5_wgrad_kernel(const float *__restrict__ gy,
                                                        const float *__restrict__ x,
                                                        float *__restrict__ part, C5WgArgs p) {
    extern __shared__ float c5_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int cb_n = p.Ci / C5_WG_CI;
    const int kb = blockIdx.x / cb_n, cb = blockIdx.x - kb * cb_n;
    const int k0 = kb * 64, c0 = cb * C5_WG_CI;
    const int s = blockIdx.y;
    const int G = p.N * p.Ho;                                   // output rows
    const int nch_all = (G + p.grc - 1) / p.grc;
    const int cbeg = s * p.cps;
    const int nchunk = min(p.cps, nch_all - cbeg);
    const int rpi = 2 * p.Ho + 3, RS = 2 * p.Wo + 3, PL = p.Wo + 2;
    const int WoP = (p.Wo + 1) & ~1;
    const int STAGE = 64 * p.ast + C5_WG_CI * p.patch;
    const int plane = p.H * p.W, HoWo = p.Ho * p.Wo;

    // gy loads: thread -> pixel slot tid % pw of the chunk, channels tid / pw + (256 / pw) k
    const int pw = p.cp > 64 ? 128 : 64;
    const int apl = tid & (pw - 1), aco = tid / pw, acs = C5_T / pw, ank = 64 / acs;
    const int agl = apl / WoP, aow = apl - agl * WoP;

    float ga[C5_WG_NA];
    float gx[C5_WG_CI][C5_EMAX_WG];
    int S0 = 0, npatch = 0;                     // of the chunk held in registers
    auto gload = [&](int c) {
        const int gbeg = (cbeg + min(c, nchunk - 1)) * p.grc;
        const int gend = min(G, gbeg + p.grc);
        {
            const int gg = gbeg + agl;
            const bool ok = apl < p.cp && gg < gend && aow < p.Wo;
            const int n = ok ? gg / p.Ho : 0, oh = ok ? gg - n * p.Ho : 0;
            const float *src = gy + ((int64_t)n * p.Co + k0 + aco) * HoWo + oh * p.Wo + aow;
#pragma unroll
            for (int k = 0; k < C5_WG_NA; ++k)
                ga[k] = (ok && k < ank) ? src[(int64_t)k * acs * HoWo] : 0.f;
        }
        const int gl = gend - 1;
        S0 = (gbeg / p.Ho) * rpi + 2 * (gbeg % p.Ho);
        npatch = ((gl / p.Ho) * rpi + 2 * (gl % p.Ho) + 5 - S0) * RS;
        if (npatch > p.patch || npatch > C5_EMAX_WG * C5_T) npatch = 0;   // (host bound: never)
#pragma unroll
        for (int k = 0; k < C5_EMAX_WG; ++k) {
            const int e = tid + C5_T * k;
            int off = -1;
            if (e < npatch) {
                const int sr = S0 + e / RS, q = e % RS;
                const int n = sr / rpi, ih = sr - n * rpi - p.pt;
                const int iw = (q < PL ? 2 * q : 2 * (q - PL) + 1) - p.pl;
                if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
                    off = (n * p.Ci + c0) * plane + ih * p.W + iw;
            }
#pragma unroll
            for (int ch = 0; ch < C5_WG_CI; ++ch)
                gx[ch][k] = off >= 0 ? x[(int64_t)off + (int64_t)ch * plane] : 0.f;
        }
    };
    auto lstore = [&](int buf) {
        float *As_ = c5_lds + buf * STAGE;
        float *Bs_ = As_ + 64 * p.ast;
        if (apl < p.cp) {
#pragma unroll
            for (int k = 0; k < C5_WG_NA; ++k)
                if (k < ank) As_[(aco + k * acs) * p.ast + apl] = ga[k];
        }
#pragma unroll
        for (int k = 0; k < C5_EMAX_WG; ++k) {
            const int e = tid + C5_T * k;
            if (e < npatch) {
#pragma unroll
                for (int ch = 0; ch < C5_WG_CI; ++ch) Bs_[ch * p.patch + e] = gx[ch][k];
            }
        }
    };

    const int mh = w >> 1, ch2 = w & 1, h = lane >> 5, l32 = lane & 31;
    // column (ci, kh, kw) of group ch2 + 2 k: its fixed offset into the patch
    int lb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = min((ch2 + 2 * k) * 32 + l32, C5_WG_COLS - 1);
        const int ci = col / 25, tap = col - 25 * ci, kh = tap / 5, kw = tap - 5 * kh;
        lb[k] = ci * p.patch + kh * RS + (kw & 1) * PL + (kw >> 1);
    }
    const int arow = (mh * 32 + l32) * p.ast;
    f32x16 acc[4] = {f32x16{}, f32x16{}, f32x16{}, f32x16{}};

    if (nchunk > 0) {
        gload(0);
        lstore(0);
        __syncthreads();
    }
    for (int c = 0; c < nchunk; ++c) {
        // the geometry of chunk c (gload(c + 1) overwrites S0)
        const int gbeg = (cbeg + c) * p.grc;
        const int nrows = min(G, gbeg + p.grc) - gbeg;
        const int S0c = (gbeg / p.Ho) * rpi + 2 * (gbeg % p.Ho);
        gload(c + 1);
        const float *As_ = c5_lds + (c & 1) * STAGE + arow;
        const float *Bs_ = As_ - arow + 64 * p.ast;
        int n = gbeg / p.Ho, oh = gbeg - n * p.Ho;
        for (int gl = 0; gl < nrows; ++gl) {
            const float *ar = As_ + gl * WoP;
            const float *br = Bs_ + (n * rpi + 2 * oh - S0c) * RS;
            for (int t = 0; t < WoP; t += 2) {
                const int pix = t + h;
                const bool ok = pix < p.Wo;
                const float av = ar[pix];                       // zero past the row's end
                const float *bq = br + (ok ? pix : p.Wo - 1);
                const float b0 = ok ? bq[lb[0]] : 0.f, b1 = ok ? bq[lb[1]] : 0.f;
                const float b2 = ok ? bq[lb[2]] : 0.f, b3 = ok ? bq[lb[3]] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b2, acc[2], 0, 0, 0);
                if (ch2 == 0) acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b3, acc[3], 0, 0, 0);
            }
            if (++oh == p.Ho) {
                oh = 0;
                ++n;
            }
        }
        if (c + 1 < nchunk) {
            lstore((c + 1) & 1);
            __syncthreads();
        }
    }
    float *o = part + (int64_t)s * p.Co * p.Ci * 25;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = (ch2 + 2 * k) * 32 + l32;
        if (col >= C5_WG_COLS) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = k0 + mh * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float *d = o + ((int64_t)m * p.Ci + c0) * 25 + col;
            *d = p.accum ? *d + acc[k][r] : acc[k][r];
        }
    }
}

bool c5_aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// most staged rows x row length of a run of 64 pixels (or `rows` whole pixel
// rows) of an Hp x Wp grid: rstep rows per pixel row, krows per tap column,
// rpi per image
int c5_patch(int Hp, int Wp, int rpi, int rstep, int krows, int RS, int rows = 0) {
    const int gr = rows ? rows : (63 + Wp - 1) / Wp + 1;
    const int bnd = (gr - 1 + Hp - 1) / Hp;                   // image boundaries crossed
    return (rstep * (gr - 1) + krows + bnd * (rpi - rstep * Hp)) * RS;
}

int c5_fwd_patch(int Ho, int Wo) { return c5_patch(Ho, Wo, 2 * Ho + 3, 2, 5, 2 * Wo + 3); }

int c5_dx_patch(int H, int W) {
    // the phases' grids are the floor and ceiling halves; the largest patch of the four
    int best = 0;
    for (int Hp = H / 2; Hp <= (H + 1) / 2; ++Hp)
        for (int Wp = W / 2; Wp <= (W + 1) / 2; ++Wp)
            if (Hp > 0 && Wp > 0) best = max(best, c5_patch(Hp, Wp, Hp + 2, 1, 3, Wp + 2));
    return best;
}

int c5_wg_rows(int Wo) { return Wo >= 64 ? 1 : 64 / Wo; }

int c5_wg_patch(int Ho, int Wo) {
    return c5_patch(Ho, Wo, 2 * Ho + 3, 2, 5, 2 * Wo + 3, c5_wg_rows(Wo));
}

constexpr int C5_CUS = 256;

int c5_fwd_slices(int n, int cin, int cout, int Ho, int Wo) {
    const int64_t tiles = ((int64_t)n * Ho * Wo + 63) / 64 * (cout / 64);
    return tiles >= C5_CUS ? 1 : slab_slices((int)tiles, cin / C5_CC_FWD, 4);
}

int c5_dx_tiles(int n, int H, int W) { return (int)(((int64_t)n * ((H + 1) / 2) * ((W + 1) / 2) + 63) / 64); }

int c5_dx_slices(int n, int cin, int cout, int H, int W) {
    const int64_t tiles = (int64_t)c5_dx_tiles(n, H, W) * 4 * (cin / 64);
    return tiles >= C5_CUS ? 1 : slab_slices((int)tiles, cout / C5_CC_DX, 4);
}

// output rows per chunk: about 64 pixels, fewer where that leaves the (co, ci)
// blocks alone short of the CUs and the rows can be split over more slices
int c5_wg_chunk_rows(int n, int cin, int cout, int Ho, int Wo) {
    const int blocks = (cout / 64) * (cin / C5_WG_CI);
    const int want = (C5_CUS + blocks - 1) / blocks;
    const int64_t G = (int64_t)n * Ho;
    return (int)max((int64_t)1, min((int64_t)c5_wg_rows(Wo), (G + want - 1) / want));
}

int c5_wg_slices(int n, int cin, int cout, int Ho, int Wo) {
    const int grc = c5_wg_chunk_rows(n, cin, cout, Ho, Wo);
    return slab_slices((cout / 64) * (cin / C5_WG_CI), ((int64_t)n * Ho + grc - 1) / grc, 1);
}

size_t c5_slab_bytes(int S, int64_t n) {
    return S > 1 ? (size_t)(S + slab_groups(S)) * n * sizeof(float) : 0;
}

constexpr size_t C5_LDS_MAX = 160 * 1024;
size_t c5_fwd_lds(int Ho, int Wo) {
    return 2 * (size_t)(64 * C5_AS_FWD + C5_CC_FWD * c5_fwd_patch(Ho, Wo)) * sizeof(float);
}
size_t c5_dx_lds(int H, int W) {
    return 2 * (size_t)(64 * C5_AS_DX + C5_CC_DX * c5_dx_patch(H, W)) * sizeof(float);
}
size_t c5_wg_lds(int Ho, int Wo) {
    const int ast = (c5_wg_rows(Wo) * ((Wo + 1) & ~1)) | 1;
    return 2 * (size_t)(64 * ast + C5_WG_CI * c5_wg_patch(Ho, Wo)) * sizeof(float);
}

// the kernels take their LDS size per launch, up to the whole CU's
smmd_status c5_allow_lds(const void *k, bool &done) {
    if (done) return SMMD_OK;
    const smmd_status e = hip_status(hipFuncSetAttribute(
        k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C5_LDS_MAX));
    done = e == SMMD_OK;
    return e;
}

// the shapes all three directions tile
bool c5_ok(int n, int cin, int cout, int H, int W, int Ho, int Wo, int pt, int pl) {
    if (n <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return false;
    if (cin % 64 || cout % 64 || pt < 0 || pl < 0 || pt > 4 || pl > 4) return false;
    const int64_t lim = 1ll << 29;
    if ((int64_t)n * cin * H * W >= lim || (int64_t)n * cout * Ho * Wo >= lim ||
        (int64_t)cin * cout * 25 >= lim)
        return false;
    if (Wo > 1024 || W > 4096) return false;                  // (before the products below)
    return c5_fwd_patch(Ho, Wo) <= C5_EMAX_FWD * C5_T && c5_dx_patch(H, W) <= C5_EMAX_DX * C5_T &&
           c5_wg_patch(Ho, Wo) <= C5_EMAX_WG * C5_T && ((Wo + 1) & ~1) * c5_wg_rows(Wo) <= 128 &&
           c5_fwd_lds(Ho, Wo) <= C5_LDS_MAX && c5_dx_lds(H, W) <= C5_LDS_MAX &&
           c5_wg_lds(Ho, Wo) <= C5_LDS_MAX;
}

}  // namespace

}  // namespace smmd

using namespace smmd;

extern "C" int smmd_conv5s2_supported(int n, int cin, int cout, int h, int w, int pt, int pl) {
    if (h + 2 * pt < 5 || w + 2 * pl < 5) return 0;
    return c5_ok(n, cin, cout, h, w, (h + 2 * pt - 5) / 2 + 1, (w + 2 * pl - 5) / 2 + 1, pt, pl);
}

extern "C" size_t smmd_conv5s2_workspace_bytes(int n, int cin, int cout, int h, int w, int ho,
                                               int wo, int pt, int pl) {
    if (!c5_ok(n, cin, cout, h, w, ho, wo, pt, pl)) return 0;
    return c5_slab_bytes(c5_fwd_slices(n, cin, cout, ho, wo), (int64_t)n * cout * ho * wo);
}

extern "C" smmd_status smmd_conv5s2(const float *x, const float *wgt, const float *bias, float *y,
                                    int n, int cin, int cout, int h, int w, int ho, int wo, int pt,
                                    int pl, void *ws, size_t ws_bytes, smmd_stream_t stream) {
    if (!x || !wgt || !y) return SMMD_EINVAL;
    if (!c5_ok(n, cin, cout, h, w, ho, wo, pt, pl)) return SMMD_EUNSUPPORTED;
    if (!c5_aligned16(wgt)) return SMMD_EINVAL;
    const int S = c5_fwd_slices(n, cin, cout, ho, wo);
    const size_t need = smmd_conv5s2_workspace_bytes(n, cin, cout, h, w, ho, wo, pt, pl);
    if (need && (!ws || ws_bytes < need || !c5_aligned16(ws))) return SMMD_EWORKSPACE;
    const int nch = cin / C5_CC_FWD;
    C5Args p{};
    p.N = n; p.R = cin; p.M = cout; p.H = h; p.W = w; p.Ho = ho; p.Wo = wo; p.pt = pt; p.pl = pl;
    p.patch = c5_fwd_patch(ho, wo);
    p.cps = (nch + S - 1) / S;
    p.nslices = (nch + p.cps - 1) / p.cps;
    p.slab = (long long)n * cout * ho * wo;
    const size_t lds = c5_fwd_lds(ho, wo);
    static bool attr = false;
    smmd_status e = c5_allow_lds(reinterpret_cast<const void *>(c5_fwd_kernel), attr);
    if (e != SMMD_OK) return e;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t tiles = (p.slab / cout + 63) / 64;
    float *part = p.nslices > 1 ? static_cast<float *>(ws) : y;
    c5_fwd_kernel<<<dim3((unsigned)(tiles * (cout / 64)), (unsigned)p.nslices), dim3(C5_T), lds, st>>>(
        wgt, x, bias, part, p);
    e = last_launch_status();
    if (e != SMMD_OK || p.nslices == 1) return e;
    return slab_sum<C5FwdSum>(part, p.nslices, S, p.slab / 4, y, 0, st);
}

extern "C" size_t smmd_conv5s2_filter_bytes(int cout, int cin) {
    return (size_t)cout * cin * 25 * sizeof(float);
}

extern "C" smmd_status smmd_conv5s2_filter(const float *wgt, int cout, int cin, float *wt,
                                           size_t wt_bytes, smmd_stream_t stream) {
    if (!wgt || !wt) return SMMD_EINVAL;
    if (cout <= 0 || cin <= 0 || cout % 64 || cin % 64 || (int64_t)cin * cout * 25 >= (1ll << 29))
        return SMMD_EUNSUPPORTED;
    if (wt_bytes < smmd_conv5s2_filter_bytes(cout, cin)) return SMMD_EWORKSPACE;
    if (!c5_aligned16(wt)) return SMMD_EINVAL;
    const int64_t total = (int64_t)cout * cin * 25;
    c5_filter_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream)>>>(wgt, wt, cout, cin);
    return last_launch_status();
}

extern "C" size_t smmd_conv5s2_dx_workspace_bytes(int n, int cin, int cout, int h, int w, int ho,
                                                  int wo, int pt, int pl) {
    if (!c5_ok(n, cin, cout, h, w, ho, wo, pt, pl)) return 0;
    return c5_slab_bytes(c5_dx_slices(n, cin, cout, h, w), (int64_t)n * cin * h * w);
}

extern "C" smmd_status smmd_conv5s2_dx(const float *gy, const float *wt, float *gx, int n, int cin,
                                       int cout, int h, int w, int ho, int wo, int pt, int pl,
                                       void *ws, size_t ws_bytes, smmd_stream_t stream) {
    if (!gy || !wt || !gx) return SMMD_EINVAL;
    if (!c5_ok(n, cin, cout, h, w, ho, wo, pt, pl)) return SMMD_EUNSUPPORTED;
    if (!c5_aligned16(wt)) return SMMD_EINVAL;
    const int S = c5_dx_slices(n, cin, cout, h, w);
    const size_t need = smmd_conv5s2_dx_workspace_bytes(n, cin, cout, h, w, ho, wo, pt, pl);
    if (need && (!ws || ws_bytes < need || !c5_aligned16(ws))) return SMMD_EWORKSPACE;
    const int nch = cout / C5_CC_DX;
    C5Args p{};
    p.N = n; p.R = cout; p.M = cin; p.H = h; p.W = w; p.Ho = ho; p.Wo = wo; p.pt = pt; p.pl = pl;
    p.patch = c5_dx_patch(h, w);
    p.cps = (nch + S - 1) / S;
    p.nslices = (nch + p.cps - 1) / p.cps;
    p.slab = (long long)n * cin * h * w;
    const size_t lds = c5_dx_lds(h, w);
    static bool attr = false;
    smmd_status e = c5_allow_lds(reinterpret_cast<const void *>(c5_dx_kernel), attr);
    if (e != SMMD_OK) return e;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *part = p.nslices > 1 ? static_cast<float *>(ws) : gx;
    c5_dx_kernel<<<dim3((unsigned)(c5_dx_tiles(n, h, w) * (cin / 64)), (unsigned)p.nslices, 4),
                   dim3(C5_T), lds, st>>>(wt, gy, part, p);
    e = last_launch_status();
    if (e != SMMD_OK || p.nslices == 1) return e;
    return slab_sum<C5DxSum>(part, p.nslices, S, p.slab / 4, gx, 0, st);
}

extern "C" size_t smmd_conv5s2_wgrad_workspace_bytes(int n, int cin, int cout, int h, int w, int ho,
                                                     int wo, int pt, int pl) {
    if (!c5_ok(n, cin, cout, h, w, ho, wo, pt, pl)) return 0;
    return c5_slab_bytes(c5_wg_slices(n, cin, cout, ho, wo), (int64_t)cout * cin * 25);
}

static smmd_status c5_wgrad_launch(const float *gy, const float *x, float *gw, int n, int cin,
                                   int cout, int h, int w, int ho, int wo, int pt, int pl, void *ws,
                                   size_t ws_bytes, int accum, smmd_stream_t stream) {
    if (!gy || !x || !gw) return SMMD_EINVAL;
    if (!c5_ok(n, cin, cout, h, w, ho, wo, pt, pl)) return SMMD_EUNSUPPORTED;
    if (!c5_aligned16(gw)) return SMMD_EINVAL;
    const int S = c5_wg_slices(n, cin, cout, ho, wo);
    const size_t need = smmd_conv5s2_wgrad_workspace_bytes(n, cin, cout, h, w, ho, wo, pt, pl);
    if (need && (!ws || ws_bytes < need || !c5_aligned16(ws))) return SMMD_EWORKSPACE;
    C5WgArgs p{};
    p.N = n; p.Ci = cin; p.Co = cout; p.H = h; p.W = w; p.Ho = ho; p.Wo = wo; p.pt = pt; p.pl = pl;
    p.patch = c5_wg_patch(ho, wo);
    p.grc = c5_wg_chunk_rows(n, cin, cout, ho, wo);
    p.cp = p.grc * ((wo + 1) & ~1);
    p.ast = p.cp | 1;
    const int64_t nch = ((int64_t)n * ho + p.grc - 1) / p.grc;
    p.cps = (int)((nch + S - 1) / S);
    const int Sused = (int)((nch + p.cps - 1) / p.cps);
    p.accum = Sused == 1 ? accum : 0;
    const size_t lds = c5_wg_lds(ho, wo);
    static bool attr = false;
    smmd_status e = c5_allow_lds(reinterpret_cast<const void *>(c5_wgrad_kernel), attr);
    if (e != SMMD_OK) return e;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *part = Sused > 1 ? static_cast<float *>(ws) : gw;
    c5_wgrad_kernel<<<dim3((unsigned)((cout / 64) * (cin / C5_WG_CI)), (unsigned)Sused), dim3(C5_T),
                      lds, st>>>(gy, x, part, p);
    e = last_launch_status();
    if (e != SMMD_OK || Sused == 1) return e;
    return slab_sum<C5WgSum>(part, Sused, S, (int64_t)cout * cin * 25 / 4, gw, accum, st);
}

extern "C" smmd_status smmd_conv5s2_wgrad(const float *gy, const float *x, float *gw, int n,
                                          int cin, int cout, int h, int w, int ho, int wo, int pt,
                                          int pl, void *ws, size_t ws_bytes, smmd_stream_t stream) {
    return c5_wgrad_launch(gy, x, gw, n, cin, cout, h, w, ho, wo, pt, pl, ws, ws_bytes, 0, stream);
}

extern "C" smmd_status smmd_conv5s2_wgrad_acc(const float *gy, const float *x, float *gw, int n,
                                              int cin, int cout, int h, int w, int ho, int wo,
                                              int pt, int pl, void *ws, size_t ws_bytes,
                                              smmd_stream_t stream) {
    return c5_wgrad_launch(gy, x, gw, n, cin, cout, h, w, ho, wo, pt, pl, ws, ws_bytes, 1, stream);
}
