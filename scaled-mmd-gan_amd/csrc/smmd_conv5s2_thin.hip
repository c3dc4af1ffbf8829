// smmd_conv5s2_thin.hip -- 5x5 stride-2 convolutions with a thin side (ct <= 4
// channels) on gfx950 / MI355X, fp32 NCHW: the DCGAN critics' first layer
// (Conv2d(3, dim, 5, 2), architecture.py:323-343) and the DCGAN generators'
// last (Deconv2d(dim, 3, 5, 2)), with their input and weight gradients.  The
// 5x5 stride-2 analogue of smmd_thin.hip: the wide tensor (cw channels, a
// multiple of 16) is streamed once, the thin side stays on chip, and the
// ct x 25 taps are a GEMM dimension of the f32 matrix cores
// (v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulation).
//
// Geometry (all entries): tap (kh, kw) of wide pixel (oh, ow) touches thin
// pixel (2 oh + kh - pt, 2 ow + kw - pl), zero outside [0, H) x [0, W)
// (predicated, never loaded); Ho, Wo are arguments (TF SAME on an even image is
// pt = pl = 1 with Ho = H / 2).  w is [cw, ct, 5, 5] everywhere: the critic
// layer's [cout, cin, 5, 5] and Deconv2d's [cin, cout, 5, 5].
//
//   t5_fwd    y [N, cw, Ho, Wo] = conv(x [N, ct, H, W], w) + b: the GEMM
//             [cw x K] . [K x pixels], K = 25 ct (76 for ct = 3: 38 MFMA steps).
//             Block = a band of TR output rows of one image x 64 channels.  The
//             (2 TR + 3)-row patch of the ct planes is staged in LDS once, each
//             row as its even columns then its odd ones, so the stride-2
//             fragment reads of a tap are unit-stride over the lanes.  A wave
//             keeps the filter of the block's two 32-channel row tiles
//             fragment-resident in VGPRs (2 x 38 registers) and walks 32-pixel
//             tiles of the band: the B fragment is read straight from the patch
//             at (pixel base + tap offset), once for both row tiles; no im2col
//             buffer.  The product is cw x pixels, so an accumulator row stores
//             32 consecutive pixels of one channel plane (128-byte segments),
//             bias added in registers.  The MFMA form was kept over a
//             v_pk_fma_f32 one (thin_in_kernel's pattern): at 75 taps the VALU
//             form needs 75 registers of gathered taps per pixel and 4.8 k packed
//             FMAs per pixel pair and 64 channels, the MFMA form 76 MFMAs per 32
//             pixels; the VALU form was not built or measured.
//   t5_t      y [N, ct, H, W] = sum_{c, taps} w g [N, cw, Ho, Wo] + b (the
//             transposed conv): Z [25 ct (3 row tiles) x pixels] = W^T . g with
//             K = cw, then a gather.  Block = TH output rows of one image: the
//             TH / 2 + 2 rows of g that reach them (one or two halo rows,
//             recomputed).  The B fragments are g itself, read from global
//             memory (a lane half reads 32 consecutive pixels of one channel);
//             W^T goes through LDS in chunks of 64 channels.  Z goes to LDS;
//             each thread then owns output pixels and adds its 4, 6 or 9
//             contributions (by the phase (h + pt) % 2, (w + pl) % 2) in
//             ascending tap order, then the bias; row stores.  No atomics.
//   t5_wgrad  gw [cw, ct, 5, 5] = sum_{n, oh, ow} g x: [cw x P] . [P x 25 ct],
//             K = the pixels.  Block = one image's run of bands x 64 channels;
//             per band the x patch (as in t5_fwd), the g rows [64 x pixels]
//             (odd row stride) and the pixels' patch offsets are staged in LDS;
//             wave (mt, ks) holds the 32-channel tile mt x 3 column tiles and
//             takes the pixel pairs ks, ks + KS, ...  Each wave's sum goes to
//             its own slab of the workspace; slab_sum adds the slabs in order
//             (and gw itself last for _acc).
//
// Every sum has a fixed order and every output element is written: bit-identical
// run to run, no memset.  Resource use and timings: DESIGN.md sections 3 and 5.
#include "smmd_wino_common.hpp"

namespace smmd {

namespace {

struct T5WgSum {};

constexpr int T5_T = 256;
constexpr int T5_PATCH_MAX = 15360;     // LDS floats of the staged x patch (all planes)
constexpr int T5_Z_MAX = 24576;         // LDS floats of t5_t's Z
constexpr int T5_WG_PIX = 256;          // t5_wgrad: pixels per band
constexpr size_t T5_LDS_MAX = 160 * 1024;

struct T5Args {
    int N, cw, H, W, Ho, Wo, pt, pl;
    int TR, bands;                      // output rows per band, bands per image
    int RS, PL, patch;                  // staged row length, odd plane's offset, floats per plane
    int nbpb, MT, KS, AP;               // t5_wgrad: bands per block, wave split, g row stride
};

// the patch offset of GEMM column kk = (plane, kh, kw)
__device__ __forceinline__ int t5_tapoff(int kk, const T5Args &p) {
    const int k = kk / 25, t = kk - 25 * k, kh = t / 5, kw = t - 5 * kh;
    return k * p.patch + kh * p.RS + (kw & 1) * p.PL + (kw >> 1);
}

// the receptive field of output rows [oh0, oh0 + rows) of image planes xn:
// patch row r = input row 2 oh0 + r - pt, position q = input column 2 q - pl
// (q < PL) or 2 (q - PL) + 1 - pl; zero outside the image
template <int CT>
__device__ __forceinline__ void t5_stage_patch(const float *__restrict__ xn, float *lds,
                                               const T5Args &p, int oh0, int rows) {
    const int np = (2 * rows + 3) * p.RS, plane = p.H * p.W;
    for (int e = threadIdx.x; e < np; e += T5_T) {
        const int r = e / p.RS, q = e - r * p.RS;
        const int ih = 2 * oh0 + r - p.pt;
        const int iw = (q < p.PL ? 2 * q : 2 * (q - p.PL) + 1) - p.pl;
        const bool ok = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        const int off = ih * p.W + iw;
#pragma unroll
        for (int k = 0; k < CT; ++k) lds[k * p.patch + e] = ok ? xn[k * plane + off] : 0.f;
    }
}

// ---- t5_fwd -------------------------------------------------------------
// grid (band, n, 64-channel chunk)
template <int CT>
__global__ __launch_bounds__(T5_T) void t5_fwd_kernel(const float *__restrict__ x,
                                                      const float *__restrict__ w,
                                                      const float *__restrict__ bias,
                                                      float *__restrict__ y, T5Args p) {
    constexpr int K = CT * 25, KS = (K + 1) / 2;
    extern __shared__ float t5_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const int n = blockIdx.y, c0 = blockIdx.z * 64;
    const int oh0 = blockIdx.x * p.TR, rows = min(p.TR, p.Ho - oh0), npix = rows * p.Wo;
    const int HoWo = p.Ho * p.Wo;
    t5_stage_patch<CT>(x + (int64_t)n * CT * p.H * p.W, t5_lds, p, oh0, rows);
    // the filter fragments: row tile mt, step s holds w[c0 + 32 mt + j][2 s + h]
    const bool two = c0 + 32 < p.cw;
    float a0[KS], a1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk = 2 * s + h;
        const bool kok = kk < K;
        a0[s] = (kok && c0 + j < p.cw) ? w[(c0 + j) * K + kk] : 0.f;
        a1[s] = (kok && c0 + 32 + j < p.cw) ? w[(c0 + 32 + j) * K + kk] : 0.f;
    }
    __syncthreads();
    float *yb = y + ((int64_t)n * p.cw * p.Ho + oh0) * p.Wo;
    const int ntile = (npix + 31) >> 5;
    for (int t = wv; t < ntile; t += 4) {
        const int pix = t * 32 + j, pc = min(pix, npix - 1);   // a column past the end: the last one's operands
        const int r = pc / p.Wo;
        const float *bp = t5_lds + 2 * r * p.RS + (pc - r * p.Wo);
        f32x16 acc0 = f32x16{}, acc1 = f32x16{};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            // (the padded column of an odd K reads column 0: its coefficient is zero)
            const int o0 = t5_tapoff(2 * s, p), o1 = t5_tapoff(2 * s + 1 < K ? 2 * s + 1 : 0, p);
            const float bv = bp[h ? o1 : o0];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], bv, acc0, 0, 0, 0);
            if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], bv, acc1, 0, 0, 0);
        }
        if (pix >= npix) continue;
        // lane (h, j) holds rows (r & 3) + 8 (r >> 2) + 4 h of pixel column j
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) {
            const int c = c0 + (r16 & 3) + 8 * (r16 >> 2) + 4 * h;
            if (c < p.cw) yb[(int64_t)c * HoWo + pix] = acc0[r16] + (bias ? bias[c] : 0.f);
            if (c + 32 < p.cw)
                yb[(int64_t)(c + 32) * HoWo + pix] = acc1[r16] + (bias ? bias[c + 32] : 0.f);
        }
    }
}

// ---- t5_t ---------------------------------------------------------------
struct T5TArgs {
    int N, cw, H, W, Ho, Wo, pt, pl;
    int TH, ZP;                         // output rows per block, Z row stride
};

// grid (band of TH output rows, n)
template <int CT>
__global__ __launch_bounds__(T5_T) void t5_t_kernel(const float *__restrict__ g,
                                                    const float *__restrict__ w,
                                                    const float *__restrict__ bias,
                                                    float *__restrict__ y, T5TArgs p) {
    constexpr int ZR = CT * 25, MT = (ZR + 31) / 32, WL = MT * 32 + 1;
    extern __shared__ float t5_lds[];
    float *Wl = t5_lds;                 // [64 channels][WL]: W^T of the chunk, zero past ZR
    float *Z = t5_lds + 64 * WL;        // [ZR][ZP]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const int n = blockIdx.y;
    const int h0 = blockIdx.x * p.TH, h1 = min(p.H, h0 + p.TH);
    // the rows of g that reach output rows [h0, h1)
    const int lo = h0 + p.pt - 4;
    const int oh_lo = lo <= 0 ? 0 : (lo + 1) >> 1;
    const int oh_hi = min(p.Ho - 1, (h1 - 1 + p.pt) >> 1);
    const int npix = max(0, oh_hi - oh_lo + 1) * p.Wo;
    const int HoWo = p.Ho * p.Wo;
    const float *gn = g + ((int64_t)n * p.cw * p.Ho + oh_lo) * p.Wo;
    const int ntile = (npix + 31) >> 5, nround = (ntile + 3) >> 2;
    const int nchunk = (p.cw + 63) >> 6;
    for (int rd = 0; rd < nround; ++rd) {
        const int t = rd * 4 + wv;
        const bool live = t < ntile;
        const int pix = t * 32 + j, pc = min(pix, npix - 1);
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x16{};
        for (int ch = 0; ch < nchunk; ++ch) {
            const int c0 = ch * 64, ck = min(64, p.cw - c0);
            if (nchunk > 1 || rd == 0) {
                __syncthreads();        // the previous chunk's readers are done
                for (int e = threadIdx.x; e < ck * (MT * 32); e += T5_T) {
                    const int cc = e / (MT * 32), jj = e - cc * (MT * 32);
                    Wl[cc * WL + jj] = jj < ZR ? w[(c0 + cc) * ZR + jj] : 0.f;
                }
                __syncthreads();
            }
            if (live) {
                const float *gp = gn + (int64_t)(c0 + h) * HoWo + pc;
                const float *ap = Wl + h * WL + j;
#pragma unroll 8
                for (int s = 0; s < ck / 2; ++s) {
                    const float bv = gp[(int64_t)2 * s * HoWo];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * WL + mt * 32], bv,
                                                                       acc[mt], 0, 0, 0);
                }
            }
        }
        if (live && pix < npix) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r16 = 0; r16 < 16; ++r16) {
                    const int jr = mt * 32 + (r16 & 3) + 8 * (r16 >> 2) + 4 * h;
                    if (jr < ZR) Z[jr * p.ZP + pix] = acc[mt][r16];
                }
        }
    }
    __syncthreads();
    // the gather: output (k, hh, wq) adds its taps kh = (hh + pt) % 2, + 2, ...,
    // kw likewise, in ascending order
    const int rows = h1 - h0, nout = CT * rows * p.W;
    for (int e = threadIdx.x; e < nout; e += T5_T) {
        const int k = e / (rows * p.W), rem = e - k * rows * p.W;
        const int hl = rem / p.W, wq = rem - hl * p.W, hh = h0 + hl;
        float s = 0.f;
        for (int kh = (hh + p.pt) & 1; kh < 5; kh += 2) {
            const int oh = (hh + p.pt - kh) >> 1;
            if (hh + p.pt - kh < 0 || oh < oh_lo || oh > oh_hi) continue;
            for (int kw = (wq + p.pl) & 1; kw < 5; kw += 2) {
                const int ow = (wq + p.pl - kw) >> 1;
                if (wq + p.pl - kw < 0 || ow >= p.Wo) continue;
                s += Z[(k * 25 + kh * 5 + kw) * p.ZP + (oh - oh_lo) * p.Wo + ow];
            }
        }
        if (bias) s += bias[k];
        y[((int64_t)(n * CT + k) * p.H + hh) * p.W + wq] = s;
    }
}

// ---- t5_wgrad -----------------------------------------------------------
// grid (group of nbpb bands, n, 64-channel chunk); wave (mt, ks) writes slab
// (n groups + group) KS + ks, rows [c0 + 32 mt, + 32) of [cw][25 ct]
template <int CT>
__global__ __launch_bounds__(T5_T) void t5_wgrad_kernel(const float *__restrict__ g,
                                                        const float *__restrict__ x,
                                                        float *__restrict__ part, T5Args p) {
    constexpr int ZR = CT * 25, NT = (ZR + 31) / 32;
    extern __shared__ float t5_lds[];
    float *As = t5_lds + CT * p.patch;                      // [64][AP]
    int *pb = reinterpret_cast<int *>(As + 64 * p.AP);      // [pixels]: patch offset of a pixel
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5, j = lane & 31;
    const int n = blockIdx.y, grp = blockIdx.x, c0 = blockIdx.z * 64;
    const int mt = wv % p.MT, ks = wv / p.MT;
    const int cwb = min(64, p.cw - c0);
    int tap[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tap[nt] = t5_tapoff(min(nt * 32 + j, ZR - 1), p);
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x16{};
    const float *xn = x + (int64_t)n * CT * p.H * p.W;
    const int bend = min(p.bands, (grp + 1) * p.nbpb);
    for (int b = grp * p.nbpb; b < bend; ++b) {
        const int oh0 = b * p.TR, rows = min(p.TR, p.Ho - oh0);
        const int npix = rows * p.Wo, npe = (npix + 1) & ~1;
        __syncthreads();                                    // the previous band's readers are done
        t5_stage_patch<CT>(xn, t5_lds, p, oh0, rows);
        const float *gb = g + ((int64_t)(n * p.cw + c0) * p.Ho + oh0) * p.Wo;
        for (int e = threadIdx.x; e < 64 * npe; e += T5_T) {
            const int cc = e / npe, px = e - cc * npe;
            As[cc * p.AP + px] = (cc < cwb && px < npix) ? gb[(int64_t)cc * p.Ho * p.Wo + px] : 0.f;
        }
        for (int e = threadIdx.x; e < npe; e += T5_T) {
            const int r = e / p.Wo;
            pb[e] = e < npix ? 2 * r * p.RS + (e - r * p.Wo) : 0;   // (the padded pixel: g = 0)
        }
        __syncthreads();
        const float *ar = As + (mt * 32 + j) * p.AP + h;
        for (int s = ks; s < npe / 2; s += p.KS) {
            const float av = ar[2 * s];
            const float *bq = t5_lds + pb[2 * s + h];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bq[tap[nt]], acc[nt], 0, 0, 0);
        }
    }
    float *o = part + (int64_t)((n * gridDim.x + grp) * p.KS + ks) * p.cw * ZR;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = nt * 32 + j;
        if (col >= ZR) continue;
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) {
            const int c = c0 + mt * 32 + (r16 & 3) + 8 * (r16 >> 2) + 4 * h;
            if (c < p.cw) o[(int64_t)c * ZR + col] = acc[nt][r16];
        }
    }
}

// ---- host ---------------------------------------------------------------
bool t5_ok(int n, int ct, int cw, int H, int W, int Ho, int Wo, int pt, int pl) {
    if (n <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return false;
    if (ct < 1 || ct > 4 || cw < 16 || cw % 16 || pt < 0 || pt > 2 || pl < 0 || pl > 2) return false;
    // the last wide row's taps end on the thin image's last row, up to one row
    // short of it (a row no tap reaches) or two past it (zero taps)
    if (2 * Ho + 2 - pt < H - 2 || 2 * Ho + 2 - pt > H + 1) return false;
    if (2 * Wo + 2 - pl < W - 2 || 2 * Wo + 2 - pl > W + 1) return false;
    const int64_t lim = 1ll << 29;
    if ((int64_t)n * ct * H * W >= lim || (int64_t)n * cw * Ho * Wo >= lim ||
        (int64_t)cw * ct * 25 >= lim)
        return false;
    // one output row's patch, three rows of Z and one row of g fit their LDS stages
    return ct * 5 * (2 * Wo + 3) <= T5_PATCH_MAX && 3 * Wo + 1 <= T5_Z_MAX / (ct * 25) &&
           Wo <= T5_WG_PIX;
}

int t5_chunks(int cw) { return (cw + 63) / 64; }

// output rows per band: about want_pix pixels, within the patch stage, fewer
// while that leaves the launch short of 512 blocks and a wave a tile
int t5_rows(int n, int ct, int cw, int Ho, int Wo, int want_pix, int min_blocks) {
    const int cap = (T5_PATCH_MAX / (ct * (2 * Wo + 3)) - 3) / 2;
    int TR = max(1, min(Ho, min(cap, want_pix / Wo)));
    while (TR > 1 && (int64_t)n * ((Ho + TR - 1) / TR) * t5_chunks(cw) < min_blocks &&
           ((TR + 1) / 2) * Wo >= 128)
        TR = (TR + 1) / 2;
    return TR;
}

void t5_fill(T5Args &p, int n, int cw, int H, int W, int Ho, int Wo, int pt, int pl, int TR) {
    p.N = n; p.cw = cw; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.pt = pt; p.pl = pl;
    p.TR = TR; p.bands = (Ho + TR - 1) / TR;
    p.RS = 2 * Wo + 3; p.PL = Wo + 2; p.patch = (2 * TR + 3) * p.RS;
}

// t5_wgrad's split: bands of <= T5_WG_PIX pixels, bands per block so that the
// launch keeps about 128 blocks, KS pixel slices per block
void t5_wg_fill(T5Args &p, int n, int ct, int cw, int H, int W, int Ho, int Wo, int pt, int pl) {
    t5_fill(p, n, cw, H, W, Ho, Wo, pt, pl, t5_rows(n, ct, cw, Ho, Wo, T5_WG_PIX, 0));
    p.nbpb = (int)max((int64_t)1, (int64_t)n * p.bands * t5_chunks(cw) / 128);
    p.nbpb = min(p.nbpb, p.bands);
    p.MT = cw > 32 ? 2 : 1;
    p.KS = 4 / p.MT;
    p.AP = ((p.TR * Wo + 1) & ~1) | 1;
}

int t5_wg_groups(const T5Args &p) { return (p.bands + p.nbpb - 1) / p.nbpb; }

template <class Kern>
smmd_status t5_allow_lds(Kern k, bool &done) {
    if (done) return SMMD_OK;
    const smmd_status e = hip_status(hipFuncSetAttribute(
        reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)T5_LDS_MAX));
    done = e == SMMD_OK;
    return e;
}

template <int CT>
smmd_status t5_fwd_launch(const float *x, const float *w, const float *b, float *y,
                          const T5Args &p, hipStream_t st) {
    static bool attr = false;
    const smmd_status e = t5_allow_lds(t5_fwd_kernel<CT>, attr);
    if (e != SMMD_OK) return e;
    t5_fwd_kernel<CT><<<dim3(p.bands, p.N, t5_chunks(p.cw)), dim3(T5_T),
                        (size_t)CT * p.patch * sizeof(float), st>>>(x, w, b, y, p);
    return last_launch_status();
}

template <int CT>
smmd_status t5_t_launch(const float *g, const float *w, const float *b, float *y, T5TArgs p,
                        hipStream_t st) {
    constexpr int ZR = CT * 25, WL = (ZR + 31) / 32 * 32 + 1;
    // rows of g per block within Z's stage; TH = 2 (rows - 2), at most 8
    const int grcap = (T5_Z_MAX / ZR - 1) / p.Wo;
    p.TH = max(2, min(8, 2 * (grcap - 2)));
    p.TH = min(p.TH, (p.H + 1) & ~1);
    p.ZP = ((p.TH / 2 + 2) * p.Wo) | 1;
    static bool attr = false;
    const smmd_status e = t5_allow_lds(t5_t_kernel<CT>, attr);
    if (e != SMMD_OK) return e;
    t5_t_kernel<CT><<<dim3((p.H + p.TH - 1) / p.TH, p.N), dim3(T5_T),
                      (size_t)(64 * WL + ZR * p.ZP) * sizeof(float), st>>>(g, w, b, y, p);
    return last_launch_status();
}

template <int CT>
smmd_status t5_wg_launch(const float *g, const float *x, float *part, const T5Args &p,
                         hipStream_t st) {
    static bool attr = false;
    const smmd_status e = t5_allow_lds(t5_wgrad_kernel<CT>, attr);
    if (e != SMMD_OK) return e;
    const size_t lds = (size_t)(CT * p.patch + 64 * p.AP + p.AP + 1) * sizeof(float);
    t5_wgrad_kernel<CT><<<dim3(t5_wg_groups(p), p.N, t5_chunks(p.cw)), dim3(T5_T), lds, st>>>(
        g, x, part, p);
    return last_launch_status();
}

#define T5_BY_CT(ct, call, ...)                     \
    switch (ct) {                                   \
        case 1: e = call<1>(__VA_ARGS__); break;    \
        case 2: e = call<2>(__VA_ARGS__); break;    \
        case 3: e = call<3>(__VA_ARGS__); break;    \
        default: e = call<4>(__VA_ARGS__); break;   \
    }

}  // namespace

}  // namespace smmd

using namespace smmd;

extern "C" int smmd_conv5s2_thin_supported(int n, int ct, int cw, int h, int w, int ho, int wo,
                                           int pt, int pl) {
    return t5_ok(n, ct, cw, h, w, ho, wo, pt, pl);
}

extern "C" smmd_status smmd_conv5s2_thin(const float *x, const float *wgt, const float *bias,
                                         float *y, int n, int ct, int cw, int h, int w, int ho,
                                         int wo, int pt, int pl, smmd_stream_t stream) {
    if (!x || !wgt || !y) return SMMD_EINVAL;
    if (!t5_ok(n, ct, cw, h, w, ho, wo, pt, pl)) return SMMD_EUNSUPPORTED;
    T5Args p{};
    t5_fill(p, n, cw, h, w, ho, wo, pt, pl, t5_rows(n, ct, cw, ho, wo, 512, 512));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    smmd_status e;
    T5_BY_CT(ct, t5_fwd_launch, x, wgt, bias, y, p, st)
    return e;
}

extern "C" smmd_status smmd_conv5s2_thin_t(const float *g, const float *wgt, const float *bias,
                                           float *y, int n, int ct, int cw, int h, int w, int ho,
                                           int wo, int pt, int pl, smmd_stream_t stream) {
    if (!g || !wgt || !y) return SMMD_EINVAL;
    if (!t5_ok(n, ct, cw, h, w, ho, wo, pt, pl)) return SMMD_EUNSUPPORTED;
    T5TArgs p{};
    p.N = n; p.cw = cw; p.H = h; p.W = w; p.Ho = ho; p.Wo = wo; p.pt = pt; p.pl = pl;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    smmd_status e;
    T5_BY_CT(ct, t5_t_launch, g, wgt, bias, y, p, st)
    return e;
}

extern "C" size_t smmd_conv5s2_thin_wgrad_workspace_bytes(int n, int ct, int cw, int h, int w,
                                                          int ho, int wo, int pt, int pl) {
    if (!t5_ok(n, ct, cw, h, w, ho, wo, pt, pl)) return 0;
    T5Args p{};
    t5_wg_fill(p, n, ct, cw, h, w, ho, wo, pt, pl);
    const int S = n * t5_wg_groups(p) * p.KS;
    return (size_t)(S + slab_groups(S)) * cw * ct * 25 * sizeof(float);
}

static smmd_status t5_wgrad(const float *g, const float *x, float *gw, int n, int ct, int cw, int h,
                            int w, int ho, int wo, int pt, int pl, void *ws, size_t ws_bytes,
                            int accum, smmd_stream_t stream) {
    if (!g || !x || !gw) return SMMD_EINVAL;
    if (!t5_ok(n, ct, cw, h, w, ho, wo, pt, pl)) return SMMD_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(gw) & 15) != 0) return SMMD_EINVAL;
    const size_t need = smmd_conv5s2_thin_wgrad_workspace_bytes(n, ct, cw, h, w, ho, wo, pt, pl);
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
        return SMMD_EWORKSPACE;
    T5Args p{};
    t5_wg_fill(p, n, ct, cw, h, w, ho, wo, pt, pl);
    const int S = n * t5_wg_groups(p) * p.KS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(ws);
    smmd_status e;
    T5_BY_CT(ct, t5_wg_launch, g, x, part, p, st)
    if (e != SMMD_OK) return e;
    return slab_sum<T5WgSum>(part, S, S, (int64_t)cw * ct * 25 / 4, gw, accum, st);
}

extern "C" smmd_status smmd_conv5s2_thin_wgrad(const float *g, const float *x, float *gw, int n,
                                               int ct, int cw, int h, int w, int ho, int wo, int pt,
                                               int pl, void *ws, size_t ws_bytes,
                                               smmd_stream_t stream) {
    return t5_wgrad(g, x, gw, n, ct, cw, h, w, ho, wo, pt, pl, ws, ws_bytes, 0, stream);
}

extern "C" smmd_status smmd_conv5s2_thin_wgrad_acc(const float *g, const float *x, float *gw, int n,
                                                   int ct, int cw, int h, int w, int ho, int wo,
                                                   int pt, int pl, void *ws, size_t ws_bytes,
                                                   smmd_stream_t stream) {
    return t5_wgrad(g, x, gw, n, ct, cw, h, w, ho, wo, pt, pl, ws, ws_bytes, 1, stream);
}
