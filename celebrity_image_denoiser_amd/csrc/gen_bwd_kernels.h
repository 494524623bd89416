// gen_bwd_kernels.h — gfx950 device kernels of the DenoiseGenerator backward pass (cid_backward, include/cid.h): the gradients of the
// 24 parameter tensors and of the input (reference backend/trainingcode/denoise_gan_code/training.py:59-74) from grad_out, the tanh
// output y and the activation arena cid_forward_saved kept.
//
// Tensors are fp32 NHWC views of the arena or of the backward workspace: element (n, y, x, c) of a view (p, ps, coff) over H x W is
// p[((n*H + y)*W + x)*ps + coff + c], all offsets 64-bit.  Every sum over pixels or images accumulates in fp64 in a fixed order, no
// atomics; the GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32).  Weights are read from the blob's reference-layout copy.
//
// Every gradient of an activation is stored ONCE, finished: a data-gradient kernel multiplies by the ReLU mask (a > 0 of the stored
// activation) in its epilogue, so the weight-gradient kernel and the next data-gradient kernel stage a plain dz.  The two places
// where a gradient has two sources (e1 / e2: max-pool routing plus the concat's skip slice) are finished by k_gen_pool_bwd, in place
// in the skip slice of the concat gradient.
//   * k_gen_dz16: dz of the last layer, grad_out * (1 - y^2), NCHW.
//   * k_gen_dgrad<CD, CXB, TAPS>: data gradient in gather form of a 3x3 convolution (TAPS 9: the full correlation with flipped taps,
//     zero padding) or of a 2x2 stride-2 transposed convolution (TAPS 4: every dz pixel belongs to one (input pixel, tap), K = 4 CD).
//     A workgroup owns a tile of output pixels and CXB channels; contraction over 8-channel chunks of dz.
//   * k_gen_wgrad<CRB, CONVT> + k_gen_wgrad_reduce: weight gradient as a GEMM contracted over pixels.  "Row" operand: the tensor
//     read at the pixel itself (dz of a convolution; the INPUT of a transposed convolution), CRB channels per workgroup; "column"
//     operand: the tensor read at the tap's offset (the input of a convolution; dz of a transposed convolution), 16 channels per
//     workgroup.  A workgroup keeps its [CRB x TAPS*16] tile in registers over a contiguous range of (image, 4 x 16 pixel) items and
//     writes one partial tile; the reduce kernel sums the partials in fp64 in a fixed order.  Bias gradients ride along.
//   * k_gen_wgrad27<TAIL> + k_gen_wgrad27_reduce<TAIL>, k_gen_dgrad_tail, k_gen_dgrad_head: the two K = 27 layers on the VALU
//     (upconv1.2: 64 -> 3 and down1.0: 3 -> 64); the pixel sums in fp64.
//   * k_gen_pool_bwd<C>: dz of a skip tensor e = (max-pool routing of dp + skip gradient) * (e > 0); the routed element is the first in
//     window scan order (0,0), (0,1), (1,0), (1,1) that equals the window's maximum (ATen's rule).
#pragma once
#include "disc_kernels.h"

namespace cid {

constexpr int G_THREADS = 256;
constexpr int G_TW = 16;   // pixels per tile row (one MFMA column tile)

// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(G_THREADS) k_gen_dz16(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ dz,
                                                        long long total) {
    const long long i = (long long)blockIdx.x * G_THREADS + threadIdx.x;
    if (i < total) {
        const float t = y[i];
        dz[i] = g[i] * (1.0f - t * t);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Data gradient.  TAPS 9: out[n, y, x, ci] = sum_{co, kh, kw} dz[n, y+1-kh, x+1-kw, co] * W[co, ci, kh, kw], W = [CD][CX][3][3].
//                 TAPS 4: out[n, y, x, ci] = sum_{co, kh, kw} dz[n, 2y+kh, 2x+kw, co] * W[ci, co, kh, kw],   W = [CX][CD][2][2].
// Then out *= (act > 0) when act is given.
struct GenDgradArgs {
    const float* dz; int dz_ps, dz_coff;      // CD channels; TAPS 9: H x W, TAPS 4: 2H x 2W
    const float* w;                           // reference layout
    const float* act; int act_ps, act_coff;   // the stored activation whose gradient this is (H x W, CX channels), or null
    float* out; int out_ps, out_coff;         // CX channels, H x W
    int H, W, CX;
    int tiles_x, tiles;                       // tiles per image
    int n0;
};

template <int CXB, int TAPS>
struct GenDgradGeom {
    static constexpr int WN = CXB / 64;
    static constexpr int WM = 4 / WN;
    static constexpr int TH = 4 * WM;                                   // tile rows
    static constexpr int HH = TAPS == 9 ? TH + 2 : TH;
    static constexpr int HWD = TAPS == 9 ? G_TW + 2 : G_TW;
    static constexpr int NPIX = HH * HWD;
    static constexpr int XSTR = NPIX + ((16 - NPIX % 32) + 32) % 32;    // 16 mod 32: planes k and k+1 on disjoint banks
    static constexpr int PLANES = TAPS == 9 ? 8 : 32;                   // TAPS 4: one plane per (tap, channel)
    static constexpr int WSTR = CXB + 16;
    static_assert(CXB == 64 || CXB == 128, "64 channels per wave");
    static_assert(TAPS == 9 || TAPS == 4, "3x3 convolution or 2x2 transposed convolution");
};

template <int CD, int CXB, int TAPS>
__global__ void __launch_bounds__(G_THREADS, 2) k_gen_dgrad(const GenDgradArgs a) {
    using G = GenDgradGeom<CXB, TAPS>;
    constexpr int WM = G::WM, TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[G::PLANES * XSTR];
    __shared__ float lds_w[TAPS * 8 * WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l16 = lane & 15, kq = lane >> 4;
    const int cb = blockIdx.x / a.tiles, t = blockIdx.x - cb * a.tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int i0 = ty * TH, j0 = tx * G_TW;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int Hd = TAPS == 9 ? a.H : 2 * a.H, Wd = TAPS == 9 ? a.W : 2 * a.W;
    const float* dzn = a.dz + n * (size_t)Hd * Wd * a.dz_ps + a.dz_coff;

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int wb = kq * WSTR + wn * 64 + l16;

    for (int chunk = 0; chunk < CD / 8; ++chunk) {
        __syncthreads();
        // ---- dz of this chunk's 8 channels -> LDS planes
        if constexpr (TAPS == 9) {
            for (int idx = tid; idx < NPIX * 2; idx += G_THREADS) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int oy = i0 - 1 + hy, ox = j0 - 1 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (oy >= 0 && oy < Hd && ox >= 0 && ox < Wd)
                    v = *reinterpret_cast<const d_f32x4*>(dzn + ((size_t)oy * Wd + ox) * a.dz_ps + chunk * 8 + h * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        } else {
            // the 2TH x 32 dz pixels under the tile: pixel (ry, rx) is tap (ry & 1, rx & 1) of tile pixel (ry / 2, rx / 2)
            for (int idx = tid; idx < TH * 2 * G_TW * 2 * 2; idx += G_THREADS) {
                const int q = idx >> 1, h = idx & 1;
                const int ry = q / (2 * G_TW), rx = q - ry * (2 * G_TW);
                const int oy = 2 * i0 + ry, ox = 2 * j0 + rx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (oy < Hd && ox < Wd) v = *reinterpret_cast<const d_f32x4*>(dzn + ((size_t)oy * Wd + ox) * a.dz_ps + chunk * 8 + h * 4);
                const int tap = (ry & 1) * 2 + (rx & 1), p = (ry >> 1) * G_TW + (rx >> 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(tap * 8 + h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights: row (tap, dz channel) holds the CXB output channels of this block
        for (int i = tid; i < 8 * CXB; i += G_THREADS) {
            const int ci = i % CXB, coj = i / CXB;
            const float* src = TAPS == 9 ? a.w + ((size_t)(chunk * 8 + coj) * a.CX + cb * CXB + ci) * 9
                                         : a.w + ((size_t)(cb * CXB + ci) * CD + chunk * 8 + coj) * 4;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) lds_w[(tap * 8 + coj) * WSTR + ci] = src[tap];
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                float av[4], bv[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) av[ct] = lds_w[wb + (tap * 8 + sub * 4) * WSTR + ct * 16];
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) {
                    if constexpr (TAPS == 9)   // tap (kh, kw) reads halo row r + 2 - kh, column c + 2 - kw
                        bv[pt] = lds_x[(sub * 4 + kq) * XSTR + (wm * 4 + pt + 2 - tap / 3) * HWD + l16 + 2 - tap % 3];
                    else
                        bv[pt] = lds_x[(tap * 8 + sub * 4 + kq) * XSTR + (wm * 4 + pt) * G_TW + l16];
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
    }

    // a lane holds channels 4 kq .. 4 kq + 3 of channel tile ct for pixel (row wm*4 + pt, column l16)
    const int x = j0 + l16;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int y = i0 + wm * 4 + pt;
        if (y < a.H && x < a.W) {
            const size_t pix = (n * a.H + y) * (size_t)a.W + x;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int ci = cb * CXB + wn * 64 + ct * 16 + kq * 4;
                d_f32x4 v = acc[ct][pt];
                if (a.act) {
                    const d_f32x4 m = *reinterpret_cast<const d_f32x4*>(a.act + pix * a.act_ps + a.act_coff + ci);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.0f ? v[e] : 0.0f;
                }
                *reinterpret_cast<d_f32x4*>(a.out + pix * a.out_ps + a.out_coff + ci) = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Weight gradient.  Row operand r (R channels, Hr x Wr, read at the item's pixels), column operand c (C channels):
//   convolution            dW[co = row][ci = col][kh][kw] = sum r[n, y, x, row] * c[n, y+kh-1, x+kw-1, col]      (c: Hr x Wr, zero padded)
//   transposed convolution dW[ci = row][co = col][kh][kw] = sum r[n, y, x, row] * c[n, 2y+kh, 2x+kw, col]        (c: 2Hr x 2Wr)
// Bias gradient: the per-channel sum of dz, which is r for a convolution and c for a transposed convolution.
struct GenWgradArgs {
    const float* r; int r_ps, r_coff; int Hr, Wr, R;
    const float* c; int c_ps, c_coff; int C;
    float* part;           // out: part[(((split*(C/16) + cblk)*R + row)*TAPS + tap)*16 + col%16]
    double* part_b;        // out: part_b[split*NB + channel], NB = R (convolution) or C (transposed convolution)
    long long items;       // N * tiles
    int splits;
    int tiles_x, tiles;
};

constexpr int G_WG_TH = 4;   // pixel rows per item: the four k of one MFMA

template <bool CONVT>
struct GenWgradGeom {
    static constexpr int S = CONVT ? 2 : 1, KH = CONVT ? 2 : 3, PAD = CONVT ? 0 : 1, TAPS = KH * KH;
    static constexpr int HH = (G_WG_TH - 1) * S + KH;
    static constexpr int HWD = (G_TW - 1) * S + KH;
    // B operand read: lanes 0-15 are 16 channel planes, lanes 16-31 the same planes one k (S halo rows) further.  S = 1: plane
    // stride 2 mod 32 and an odd row stride; S = 2: plane stride 1 mod 32 and a row stride of 8 mod 16.
    static constexpr int RS = CONVT ? 40 : HWD + 1;
    static constexpr int NP = HH * RS;
    static constexpr int XSTR = NP + (((CONVT ? 1 : 2) - NP % 32) + 32) % 32;
    static constexpr int ZSTR = G_WG_TH * G_TW + 1;   // A operand: channel stride 1 mod 32, k stride 16
    static_assert(RS >= HWD, "row stride");
};

// Known limit, open ("fp32 weight-gradient chains that grow with N"): a workgroup's whole range of items is one
// fp32 accumulation chain, as k_disc_wgrad's was before D_WG_CHUNK (disc_bwd_kernels.h); no test runs it at an N where that shows.
template <int CRB, bool CONVT>
__global__ void __launch_bounds__(G_THREADS, 2) k_gen_wgrad(const GenWgradArgs a) {
    using G = GenWgradGeom<CONVT>;
    constexpr int S = G::S, KH = G::KH, PAD = G::PAD, TAPS = G::TAPS, HH = G::HH, HWD = G::HWD, RS = G::RS, XSTR = G::XSTR, ZSTR = G::ZSTR;
    constexpr int RT = CRB / 64;   // 16-channel row tiles per wave
    __shared__ float lds_a[16 * XSTR];
    __shared__ float lds_z[CRB * ZSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, blk = blockIdx.y, rb = blockIdx.z;
    const long long it0 = a.items * split / a.splits, it1 = a.items * (split + 1) / a.splits;
    const int Hc = S * a.Hr, Wc = S * a.Wr;

    d_f32x4 acc[RT][TAPS];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) acc[r][tap] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    double bsum = 0.0;

    const int zb = ((wave * RT) * 16 + l16) * ZSTR + kq * G_TW;
    const int ab = l16 * XSTR + kq * S * RS;

    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.tiles);
        const int t = (int)(item - (long long)n * a.tiles), ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const int y0 = ty * G_WG_TH, x0 = tx * G_TW;
        const int cy0 = y0 * S - PAD, cx0 = x0 * S - PAD;
        __syncthreads();   // every wave is done with the previous item
        // ---- row operand tile: CRB channels x 4 x 16 pixels (0 outside the tensor)
        const float* rn = a.r + n * (size_t)a.Hr * a.Wr * a.r_ps + a.r_coff + rb * CRB;
        for (int idx = tid; idx < CRB * 16; idx += G_THREADS) {
            // q: group of 4 channels, p: pixel of the tile; 8 lanes read 32 consecutive channels (128 bytes) of a pixel, and the
            // 32 lanes of a half wave write 32 different banks (channel stride 1 mod 32)
            const int p = (idx >> 3) & 63, q = (idx >> 9) * 8 + (idx & 7);
            const int r = p >> 4, c = p & 15;
            const int y = y0 + r, x = x0 + c;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (y < a.Hr && x < a.Wr) v = *reinterpret_cast<const d_f32x4*>(rn + ((size_t)y * a.Wr + x) * a.r_ps + q * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_z[(q * 4 + j) * ZSTR + p] = v[j];
        }
        // ---- halo of the 16 column-operand channels of this block (0 outside the tensor)
        const float* cn = a.c + n * (size_t)Hc * Wc * a.c_ps + a.c_coff + blk * 16;
        for (int idx = tid; idx < HH * HWD * 4; idx += G_THREADS) {
            const int q = idx & 3, p = idx >> 2;
            const int hy = p / HWD, hx = p - hy * HWD;
            const int y = cy0 + hy, x = cx0 + hx;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (y >= 0 && y < Hc && x >= 0 && x < Wc) v = *reinterpret_cast<const d_f32x4*>(cn + ((size_t)y * Wc + x) * a.c_ps + q * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_a[(q * 4 + j) * XSTR + hy * RS + hx] = v[j];
        }
        __syncthreads();
        if constexpr (!CONVT) {
            if (blk == 0 && tid < CRB) {
                double s = 0.0;
                for (int i = 0; i < G_WG_TH * G_TW; ++i) s += (double)lds_z[tid * ZSTR + i];
                bsum += s;
            }
        } else {
            if (rb == 0 && tid < 16) {   // the halos of a transposed convolution tile the dz tensor: each dz pixel once
                double s = 0.0;
                for (int hy = 0; hy < HH; ++hy)
                    for (int hx = 0; hx < HWD; ++hx) s += (double)lds_a[tid * XSTR + hy * RS + hx];
                bsum += s;
            }
        }
        // ---- 16 k-steps (columns) of four pixel rows: RT x TAPS MFMAs per step per wave
#pragma unroll 4
        for (int col = 0; col < G_TW; ++col) {
            float av[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) av[r] = lds_z[zb + r * 16 * ZSTR + col];
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const float bv = lds_a[ab + (tap / KH) * RS + col * S + tap % KH];
#pragma unroll
                for (int r = 0; r < RT; ++r) acc[r][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv, acc[r][tap], 0, 0, 0);
            }
        }
    }

    // a lane holds row channels 4*kq .. 4*kq+3 of its row tile for column channel l16
    float* part = a.part + ((size_t)split * (a.C / 16) + blk) * a.R * (TAPS * 16);
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = rb * CRB + (wave * RT + r) * 16 + kq * 4 + e;
                part[((size_t)row * TAPS + tap) * 16 + l16] = acc[r][tap][e];
            }
    if constexpr (!CONVT) {
        if (blk == 0 && tid < CRB) a.part_b[(size_t)split * a.R + rb * CRB + tid] = bsum;
    } else {
        if (rb == 0 && tid < 16) a.part_b[(size_t)split * a.C + blk * 16 + tid] = bsum;
    }
}

struct GenWgradReduceArgs {
    const float* part;
    const double* part_b;
    float* dw;      // out [R][C][TAPS], may be null
    float* db;      // out [NB], may be null
    int splits, R, C, TAPS, NB;
};

__global__ void __launch_bounds__(G_THREADS) k_gen_wgrad_reduce(const GenWgradReduceArgs a) {
    const int o = blockIdx.x * G_THREADS + threadIdx.x;
    const int nw = a.R * a.C * a.TAPS;
    if (o < nw) {
        if (!a.dw) return;
        const int tap = o % a.TAPS, c = (o / a.TAPS) % a.C, row = o / (a.TAPS * a.C);
        const size_t stride = (size_t)(a.C / 16) * a.R * a.TAPS * 16;
        const float* p = a.part + (((size_t)(c >> 4) * a.R + row) * a.TAPS + tap) * 16 + (c & 15);
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += (double)p[k * stride];
        a.dw[o] = (float)s;
    } else if (o < nw + a.NB) {
        if (!a.db) return;
        const int ch = o - nw;
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += a.part_b[(size_t)k * a.NB + ch];
        a.db[ch] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The two K = 27 layers.  d: NHWC, 64 channels; src: NCHW, 3 channels; a pixel's 27 patch values k = (c3*3 + kh)*3 + kw are
//   HEAD (down1.0):   src = the network input x, d = dz of t0:   dW[co][c3][kh][kw] = sum d[p, co] * x[c3, p + (kh-1, kw-1)];  k = 27: 1 (bias)
//   TAIL (upconv1.2): src = dz16, d = the stored t4:             dW[c3][ci][kh][kw] = sum t4[p, ci] * dz16[c3, p - (kh-1, kw-1)]
//                     and the bias gradient is the sum of dz16 = of the centre taps.
// A workgroup walks a contiguous range of (image, 64-pixel strip) items; thread = (channel of d, group of 7 k); fp64 throughout.
struct GenWgrad27Args {
    const float* src;      // fp32 [N,3,H,W]
    const float* d; int d_ps, d_coff;
    double* part;          // out: part[(split*64 + ch)*28 + k]
    double* part_b;        // TAIL out: part_b[split*3 + c3]
    long long items;       // N * strips
    int splits, strips;
    int H, W;
};

template <bool TAIL>
__global__ void __launch_bounds__(G_THREADS) k_gen_wgrad27(const GenWgrad27Args a) {
    __shared__ float lds_d[64 * 64];   // [pixel][ch]
    __shared__ float lds_p[64 * 28];   // [pixel][k]
    const int tid = threadIdx.x, ch = tid & 63, kg = tid >> 6;
    const long long HW = (long long)a.H * a.W;
    const long long it0 = a.items * blockIdx.x / a.splits, it1 = a.items * (blockIdx.x + 1) / a.splits;
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double bsum = 0.0;
    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.strips);
        const long long p0 = (item - (long long)n * a.strips) * 64;
        __syncthreads();
        for (int idx = tid; idx < 64 * 16; idx += G_THREADS) {
            const int q = idx & 15, px = idx >> 4;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (p0 + px < HW) v = *reinterpret_cast<const d_f32x4*>(a.d + (n * (size_t)HW + (size_t)(p0 + px)) * a.d_ps + a.d_coff + q * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_d[px * 64 + q * 4 + j] = v[j];
        }
        for (int idx = tid; idx < 64 * 28; idx += G_THREADS) {
            const int px = idx / 28, k = idx - px * 28;
            const long long p = p0 + px;
            float v = 0.0f;
            if (p < HW) {
                if (k == 27) {
                    v = TAIL ? 0.0f : 1.0f;
                } else {
                    const int c3 = k / 9, kh = (k / 3) % 3, kw = k % 3;
                    const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
                    const int iy = TAIL ? y + 1 - kh : y + kh - 1, ix = TAIL ? x + 1 - kw : x + kw - 1;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = a.src[(n * 3 + c3) * (size_t)HW + (size_t)iy * a.W + ix];
                }
            }
            lds_p[idx] = v;
        }
        __syncthreads();
        for (int px = 0; px < 64; ++px) {
            const double d = (double)lds_d[px * 64 + ch];
#pragma unroll
            for (int j = 0; j < 7; ++j) acc[j] += d * (double)lds_p[px * 28 + kg * 7 + j];
        }
        if (TAIL && tid < 3) {
            double s = 0.0;
            for (int px = 0; px < 64; ++px) s += (double)lds_p[px * 28 + tid * 9 + 4];
            bsum += s;
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) a.part[((size_t)blockIdx.x * 64 + ch) * 28 + kg * 7 + j] = acc[j];
    if (TAIL && tid < 3) a.part_b[(size_t)blockIdx.x * 3 + tid] = bsum;
}

struct GenWgrad27ReduceArgs {
    const double* part;
    const double* part_b;
    float* dw;     // HEAD: [64][27]; TAIL: [3][64][9]; may be null
    float* db;     // HEAD: [64]; TAIL: [3]; may be null
    int splits;
};

template <bool TAIL>
__global__ void __launch_bounds__(G_THREADS) k_gen_wgrad27_reduce(const GenWgrad27ReduceArgs a) {
    const int o = blockIdx.x * G_THREADS + threadIdx.x;
    if (o < 64 * 28) {
        const int ch = o / 28, k = o - ch * 28;
        float* dst;
        if (TAIL) dst = (k == 27 || !a.dw) ? nullptr : a.dw + ((k / 9) * 64 + ch) * 9 + k % 9;
        else dst = k == 27 ? (a.db ? a.db + ch : nullptr) : (a.dw ? a.dw + ch * 27 + k : nullptr);
        if (!dst) return;
        double s = 0.0;
        for (int i = 0; i < a.splits; ++i) s += a.part[(size_t)i * 64 * 28 + o];
        *dst = (float)s;
    } else if (TAIL && o < 64 * 28 + 3 && a.db) {
        const int c3 = o - 64 * 28;
        double s = 0.0;
        for (int i = 0; i < a.splits; ++i) s += a.part_b[(size_t)i * 3 + c3];
        a.db[c3] = (float)s;
    }
}

// Data gradient of upconv1.2 with upconv1.0's ReLU mask: out[n, y, x, ci] = (t4 > 0) * sum_{c3, kh, kw} dz16[n, c3, y+1-kh, x+1-kw] * W[c3, ci, kh, kw].
// A workgroup takes 64 consecutive pixels; thread = (pixel slot, group of 4 channels).
struct GenDgradTailArgs {
    const float* dz16;    // fp32 [N,3,H,W]
    const float* w;       // [3][64][3][3]
    const float* t4;      // NHWC, 64 channels, pixel stride 64
    float* out;           // NHWC, 64 channels, pixel stride 64
    long long pixels;     // N * H * W
    int H, W;
};

__global__ void __launch_bounds__(G_THREADS) k_gen_dgrad_tail(const GenDgradTailArgs a) {
    __shared__ __attribute__((aligned(16))) float lds_w[27 * 64];   // [k = c3*9 + tap][ci]
    const int tid = threadIdx.x, q = tid & 15, slot = tid >> 4;
    for (int i = tid; i < 27 * 64; i += G_THREADS) {
        const int ci = i & 63, k = i >> 6;
        lds_w[i] = a.w[((k / 9) * 64 + ci) * 9 + k % 9];
    }
    __syncthreads();
    const long long HW = (long long)a.H * a.W;
    for (int it = 0; it < 4; ++it) {
        const long long gp = (long long)blockIdx.x * 64 + it * 16 + slot;
        if (gp >= a.pixels) continue;
        const long long n = gp / HW, p = gp - n * HW;
        const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
        d_f32x4 acc = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int oy = y + 1 - kh, ox = x + 1 - kw;
                    float d = 0.0f;
                    if (oy >= 0 && oy < a.H && ox >= 0 && ox < a.W) d = a.dz16[((size_t)n * 3 + c3) * (size_t)HW + (size_t)oy * a.W + ox];
                    const d_f32x4 wv = *reinterpret_cast<const d_f32x4*>(lds_w + (c3 * 9 + kh * 3 + kw) * 64 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[e], d, acc[e]);
                }
        const d_f32x4 m = *reinterpret_cast<const d_f32x4*>(a.t4 + (size_t)gp * 64 + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = m[e] > 0.0f ? acc[e] : 0.0f;
        *reinterpret_cast<d_f32x4*>(a.out + (size_t)gp * 64 + q * 4) = acc;
    }
}

// Input gradient: dx[n, c3, y, x] = sum_{co, kh, kw} dz0[n, y+1-kh, x+1-kw, co] * W0[co, c3, kh, kw].  One thread per pixel.
struct GenDgradHeadArgs {
    const float* dz0;   // NHWC, 64 channels, pixel stride 64
    const float* w;     // [64][3][3][3]
    float* out;         // fp32 [N,3,H,W]
    int H, W;
    int n0;
};

__global__ void __launch_bounds__(G_THREADS) k_gen_dgrad_head(const GenDgradHeadArgs a) {
    const long long HW = (long long)a.H * a.W;
    const long long p = (long long)blockIdx.x * G_THREADS + threadIdx.x;
    if (p >= HW) return;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
    typedef __attribute__((address_space(4))) const float* ConstF;
    const ConstF wc = (ConstF)a.w;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int kh = 0; kh < 3; ++kh) {
        const int oy = y + 1 - kh;
        if (oy < 0 || oy >= a.H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int ox = x + 1 - kw;
            if (ox < 0 || ox >= a.W) continue;
            const float* dp = a.dz0 + (n * (size_t)HW + (size_t)oy * a.W + ox) * 64;
            for (int q = 0; q < 16; ++q) {
                const d_f32x4 d = *reinterpret_cast<const d_f32x4*>(dp + q * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int wbase = (q * 4 + j) * 27 + kh * 3 + kw;
#pragma unroll
                    for (int c3 = 0; c3 < 3; ++c3) acc[c3] = fmaf(wc[wbase + c3 * 9], d[j], acc[c3]);
                }
            }
        }
    }
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) a.out[(n * 3 + c3) * (size_t)HW + (size_t)p] = acc[c3];
}

// ---------------------------------------------------------------------------------------------------------------------------
// dz of a skip tensor e (C channels, 2Hp x 2Wp, the [C, 2C) slice of a concat tensor): io holds the concat's skip gradient on entry
// and dz on exit, dz = (skip + (routed ? dp : 0)) * (e > 0).  Thread = (pooled pixel, group of 4 channels).
struct GenPoolBwdArgs {
    const float* e; int e_ps, e_coff;
    const float* dp;       // NHWC, C channels, pixel stride C, Hp x Wp
    float* io; int io_ps, io_coff;
    long long total;       // N * Hp * Wp * C/4
    int Hp, Wp;
};

template <int C>
__global__ void __launch_bounds__(G_THREADS) k_gen_pool_bwd(const GenPoolBwdArgs a) {
    const long long o = (long long)blockIdx.x * G_THREADS + threadIdx.x;
    if (o >= a.total) return;
    const int q = (int)(o % (C / 4));
    const long long pp = o / (C / 4);                 // pooled pixel index over N * Hp * Wp
    const int px = (int)(pp % a.Wp);
    const long long ny = pp / a.Wp;                   // n * Hp + py
    const d_f32x4 g = *reinterpret_cast<const d_f32x4*>(a.dp + (size_t)pp * C + q * 4);
    const size_t W = (size_t)a.Wp * 2;
    const size_t base = ((size_t)ny * 2) * W + (size_t)px * 2;   // (n*H + 2 py)*W + 2 px
    const size_t pix[4] = {base, base + 1, base + W, base + W + 1};
    d_f32x4 ev[4], sk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ev[k] = *reinterpret_cast<const d_f32x4*>(a.e + pix[k] * a.e_ps + a.e_coff + q * 4);
        sk[k] = *reinterpret_cast<const d_f32x4*>(a.io + pix[k] * a.io_ps + a.io_coff + q * 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float m = fmaxf(fmaxf(ev[0][j], ev[1][j]), fmaxf(ev[2][j], ev[3][j]));
        const int win = ev[0][j] == m ? 0 : ev[1][j] == m ? 1 : ev[2][j] == m ? 2 : 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = sk[k][j] + (k == win ? g[j] : 0.0f);
            sk[k][j] = ev[k][j] > 0.0f ? v : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<d_f32x4*>(a.io + pix[k] * a.io_ps + a.io_coff + q * 4) = sk[k];
}

}  // namespace cid
